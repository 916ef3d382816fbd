#include "gemm_plan.h"

namespace fx {
namespace {

// ---------------------------------------------------------------- wide tile (128 x 64), two waves per SIMD
// The 64x64 tile moves 32 KB per 64-deep stage for 0.5 MFLOP: at the f32 MFMA rate that is ~32 B/clk
// per CU, i.e. the XCD L2 bandwidth, so that kernel is L2-bound near 40 % of peak.  Here a block
// owns 128 rows x 64 cols: two 64x64 A stages (the same loaders, rows m0 and m0+64) and one B stage
// per step, 48 KB for 1 MFLOP (1.5x the intensity).  LDS: 3-slot ring of [A0 | A1 | B] images =
// 153 KB, one block per CU.  FAST operands only (chosen on the host).
// 8 waves (512 threads): wave w owns ONE 32x32 sub-tile
// (rows 32 (w>>1) of the 128, columns 32 (w&1)), 32 MFMAs per stage over two accumulators, and
// each thread stages 2 float4 per operand image (Loader NJ = 2).  PMC on the retired 4-wave form
// of this tile (one wave per SIMD, two sub-tiles each; DESIGN section 2 has the measurement): the
// matrix pipe was busy 51 % of the wave cycles, the rest waits (barrier / loads, 24 %) and issue
// of the address / select / LDS work (26 %) that one wave cannot hide behind its own MFMAs; with
// a partner wave on the SIMD, one wave's MFMAs run while the other issues or waits.
template <int AK, int BKd, int PH>
__device__ __forceinline__ void wide8_stage(const Loader<AK, true, 2>& la0, const Loader<AK, true, 2>& la1,
                                            const Loader<BKd, true, 2>& lb, const float* cur, float* wslot,
                                            int kload, const float4* rs0, const float4* rs1, const float4* rsb,
                                            unsigned ms0, unsigned ms1, unsigned msb, float4* rn0, float4* rn1,
                                            float4* rnb, unsigned& mn0, unsigned& mn1, unsigned& mnb, int ai, int wr,
                                            int wn, int li, int lh, f32x16& acc0, f32x16& acc1) {
  using LA = Loader<AK, true, 2>;
  using LB = Loader<BKd, true, 2>;
  const float* ia = cur + ai * IMG;
  const float* ib = cur + 2 * IMG;
  float4 fa[8], fb[8];
  fa[0] = LA::frag(ia, wr, li, lh, 0);
  fb[0] = LB::frag(ib, wn * 32, li, lh, 0);
  fa[1] = LA::frag(ia, wr, li, lh, 1);
  fb[1] = LB::frag(ib, wn * 32, li, lh, 1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f32x16& acc = (q & 1) ? acc1 : acc0;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].x, fb[q].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].y, fb[q].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].z, fb[q].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].w, fb[q].w, acc, 0, 0, 0);
    if (q + 2 < 8) {
      fa[q + 2] = LA::frag(ia, wr, li, lh, q + 2);
      fb[q + 2] = LB::frag(ib, wn * 32, li, lh, q + 2);
    }
    // staggered halves: waves 0-3 (PH 0) load early and store late in the stage, their SIMD
    // partners 4-7 (PH 1) the other way round, so one wave of each SIMD issues plain MFMA groups
    // while the other does its load / LDS-store work
    if (q == (PH ? 4 : 0)) la0.load(kload, rn0, mn0);
    if (q == (PH ? 5 : 1)) la1.load(kload, rn1, mn1);
    if (q == (PH ? 6 : 2)) lb.load(kload, rnb, mnb);
    if (q == (PH ? 1 : 5)) la0.store(wslot, rs0, ms0);
    if (q == (PH ? 2 : 6)) la1.store(wslot + IMG, rs1, ms1);
    if (q == (PH ? 3 : 7)) lb.store(wslot + 2 * IMG, rsb, msb);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// FX_PREC_F32S on the f32 kernel's LDS ring: the fp32 stage images stay as they are and each wave
// splits its own MFMA operands in registers (row-major A and B images only).  Per 16-deep k chunk q
// a lane takes k in [32 lh + 8 q, +8) of the 64-deep stage (two float4 reads per operand: conflict-
// free on the 68-float rows), splits the 8 values of A and of B into NP bf16x8 pieces and issues the
// NP (NP + 1) / 2 piece products on v_mfma_f32_32x32x16_bf16: 4 LDS reads per 6 MFMAs where
// pre-split images need 6, and 4 instead of 6 LDS bytes written per element.
typedef __bf16 bf16x8r __attribute__((ext_vector_type(8)));

template <int NP>
__device__ __forceinline__ void split8(const float4& lo, const float4& hi, bf16x8r* p) {
  const float e[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)e[j];
    p[0][j] = h;
    if (NP > 1) {
      const float r1 = e[j] - (float)h;
      const __bf16 m = (__bf16)r1;
      p[1][j] = m;
      if (NP > 2) p[2][j] = (__bf16)(r1 - (float)m);
    }
  }
}

template <int NP>
__device__ __forceinline__ void split_products(const bf16x8r* a, const bf16x8r* b, f32x16& acc0, f32x16& acc1) {
  if (NP > 2) {
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc1, 0, 0, 0);
  }
  if (NP > 1) {
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc1, 0, 0, 0);
  }
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc0, 0, 0, 0);
}

template <int AK, int BKd, int PH, int NP>
__device__ __forceinline__ void wide8s_stage(const Loader<AK, true, 2>& la0, const Loader<AK, true, 2>& la1,
                                             const Loader<BKd, true, 2>& lb, const float* cur, float* wslot,
                                             int kload, const float4* rs0, const float4* rs1, const float4* rsb,
                                             unsigned ms0, unsigned ms1, unsigned msb, float4* rn0, float4* rn1,
                                             float4* rnb, unsigned& mn0, unsigned& mn1, unsigned& mnb, int ai, int wr,
                                             int wn, int li, int lh, f32x16& acc0, f32x16& acc1) {
  const float* ia = cur + ai * IMG + (wr + li) * RS + 32 * lh;
  const float* ib = cur + 2 * IMG + (wn * 32 + li) * RS + 32 * lh;
  float4 fa[4][2], fb[4][2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    fa[q][0] = *reinterpret_cast<const float4*>(ia + 8 * q);
    fa[q][1] = *reinterpret_cast<const float4*>(ia + 8 * q + 4);
    fb[q][0] = *reinterpret_cast<const float4*>(ib + 8 * q);
    fb[q][1] = *reinterpret_cast<const float4*>(ib + 8 * q + 4);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bf16x8r pa[NP], pb[NP];
    split8<NP>(fa[q][0], fa[q][1], pa);
    split8<NP>(fb[q][0], fb[q][1], pb);
    if (q + 2 < 4) {
      fa[q + 2][0] = *reinterpret_cast<const float4*>(ia + 8 * (q + 2));
      fa[q + 2][1] = *reinterpret_cast<const float4*>(ia + 8 * (q + 2) + 4);
      fb[q + 2][0] = *reinterpret_cast<const float4*>(ib + 8 * (q + 2));
      fb[q + 2][1] = *reinterpret_cast<const float4*>(ib + 8 * (q + 2) + 4);
    }
    split_products<NP>(pa, pb, acc0, acc1);
    // the same staggered load / store placement as the f32 stage (two waves per SIMD)
    if (q == (PH ? 2 : 0)) {
      la0.load(kload, rn0, mn0);
      la1.load(kload, rn1, mn1);
    }
    if (q == (PH ? 3 : 1)) lb.load(kload, rnb, mnb);
    if (q == (PH ? 0 : 2)) {
      la0.store(wslot, rs0, ms0);
      la1.store(wslot + IMG, rs1, ms1);
    }
    if (q == (PH ? 1 : 3)) lb.store(wslot + 2 * IMG, rsb, msb);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int AK, int BKd, int PH, int NP = 0>
__device__ __forceinline__ void wide8_kloop(const Loader<AK, true, 2>& la0, const Loader<AK, true, 2>& la1,
                                            const Loader<BKd, true, 2>& lb, float* lds, int kt0, int kt1, int ai,
                                            int wr, int wn, int li, int lh, f32x16& acc0, f32x16& acc1) {
  const int n = kt1 - kt0;
  if (n <= 0) return;
  const int klast = (kt1 - 1) * BK;
  constexpr int SLOT = 3 * IMG;
  float4 a0x[2], a1x[2], bx[2], a0y[2], a1y[2], by[2];
  unsigned m0x, m1x, mbx, m0y, m1y, mby;
  la0.load(kt0 * BK, a0x, m0x);
  la1.load(kt0 * BK, a1x, m1x);
  lb.load(kt0 * BK, bx, mbx);
  la0.load(min((kt0 + 1) * BK, klast), a0y, m0y);
  la1.load(min((kt0 + 1) * BK, klast), a1y, m1y);
  lb.load(min((kt0 + 1) * BK, klast), by, mby);
  la0.store(lds, a0x, m0x);
  la1.store(lds + IMG, a1x, m1x);
  lb.store(lds + 2 * IMG, bx, mbx);
  la0.store(lds + SLOT, a0y, m0y);
  la1.store(lds + SLOT + IMG, a1y, m1y);
  lb.store(lds + SLOT + 2 * IMG, by, mby);
  la0.load(min((kt0 + 2) * BK, klast), a0x, m0x);
  la1.load(min((kt0 + 2) * BK, klast), a1x, m1x);
  lb.load(min((kt0 + 2) * BK, klast), bx, mbx);
  __syncthreads();
  int slot = 0;
  auto iter = [&](int i, const float4* s0, const float4* s1, const float4* sb, unsigned q0, unsigned q1, unsigned qb,
                  float4* n0, float4* n1, float4* nb, unsigned& p0, unsigned& p1, unsigned& pb) FX_INLINE {
    const int ws = slot == 0 ? 2 : slot - 1;
    if constexpr (NP == 0)
      wide8_stage<AK, BKd, PH>(la0, la1, lb, lds + slot * SLOT, lds + ws * SLOT, min((kt0 + i + 3) * BK, klast), s0,
                               s1, sb, q0, q1, qb, n0, n1, nb, p0, p1, pb, ai, wr, wn, li, lh, acc0, acc1);
    else
      wide8s_stage<AK, BKd, PH, NP>(la0, la1, lb, lds + slot * SLOT, lds + ws * SLOT, min((kt0 + i + 3) * BK, klast),
                                    s0, s1, sb, q0, q1, qb, n0, n1, nb, p0, p1, pb, ai, wr, wn, li, lh, acc0, acc1);
    __syncthreads();   // (a barrier after the next stage's first MFMA group instead measured 3 % slower)
    slot = slot == 2 ? 0 : slot + 1;
  };
  int i = 0;
  for (; i + 1 < n; i += 2) {
    iter(i, a0x, a1x, bx, m0x, m1x, mbx, a0y, a1y, by, m0y, m1y, mby);
    iter(i + 1, a0y, a1y, by, m0y, m1y, mby, a0x, a1x, bx, m0x, m1x, mbx);
  }
  if (i < n) iter(i, a0x, a1x, bx, m0x, m1x, mbx, a0y, a1y, by, m0y, m1y, mby);
}

template <int AK, int BKIND, int NP = 0>
__global__ __launch_bounds__(W8T) void gemm_f32_wide8_kernel(GemmDev g) {
  __shared__ float lds[NSLOT * 3 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  const int ai = wm >> 1, wr = (wm & 1) * 32;   // A image (rows m0 / m0 + 64) and row offset in it
  // persist: gridDim.x (a multiple of 8) workgroups walk the tiles as virtual workgroup ids blockIdx.x +
  // i gridDim.x -- same XCD as the physical one -- saving a dispatch and teardown per tile
  for (int vb = blockIdx.x;; vb += gridDim.x) {
  int tx, ty, z;
  if (g.persist) {
    if (vb >= g.persist) break;
    block_tile_id(g, vb, tx, ty);
    z = 0;
  } else {
    block_tile(g, tx, ty, z);
  }
  const int n0 = tx * BN, m0 = ty * WBM;
  const int bidx = z / g.split, sk = z - bidx * g.split;
  const int nkt = (g.K + BK - 1) / BK;
  const int kt0 = sk * g.kt_per_split;
  const int kt1 = min(nkt, kt0 + g.kt_per_split);
  Loader<AK, true, 2> la0, la1;
  Loader<BKIND, true, 2> lb;
  const float* pa = g.a.ptr + (long long)bidx * g.a.batch_stride;
  la0.init(batch_op_a(g.a, g.a_dil_b1, bidx), pa, m0, g.M, g.K, tid, g.soff, g.nsoff);
  la1.init(batch_op_a(g.a, g.a_dil_b1, bidx), pa, m0 + BM, g.M, g.K, tid, g.soff, g.nsoff);
  lb.init(batch_op_b(g.b, g.b_dil_growth, bidx), g.b.ptr + (long long)bidx * g.b.batch_stride, n0, g.N, g.K, tid, g.soff, g.nsoff);
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc0[i] = 0.f;
    acc1[i] = 0.f;
  }
  if (wave >= 4)   // the second wave of each SIMD runs the staggered stage schedule
    wide8_kloop<AK, BKIND, 1, NP>(la0, la1, lb, lds, kt0, kt1, ai, wr, wn, li, lh, acc0, acc1);
  else
    wide8_kloop<AK, BKIND, 0, NP>(la0, la1, lb, lds, kt0, kt1, ai, wr, wn, li, lh, acc0, acc1);
  const f32x16 acc = acc0 + acc1;
  const int col = n0 + wn * 32 + li;
  const int rbase = m0 + wm * 32 + 4 * lh;
  if (g.split > 1) {
    if (col < g.N) {
      float* slab = g.ws + ((long long)bidx * g.split + sk) * g.M * (long long)g.N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        if (row < g.M) slab[(long long)row * g.N + col] = acc[r];
      }
    }
    if (g.tile_cnt)
      splitk_finish<WBM, BN>(g, bidx, m0, n0, (bidx * g.tiles_y + ty) * g.tiles_x + tx,
                             reinterpret_cast<int*>(&lds[NSLOT * 3 * IMG - 1]));
    return;
  }
  tile_epilogue(g, bidx, rbase, col, acc);
  if (!g.persist) break;
  __syncthreads();   // the next tile's prologue refills the LDS ring
  }
}

}  // namespace

// np > 0 (FX_PREC_F32S / F32S2, B row-major): the same kernel splitting its operands in registers
int launch_wide8(const GemmPlan& P, hipStream_t s) {
  if (P.np == 3)
    return dispatch_pair<wide8_split_pair>(P.ak, P.bk, "wide8", [&](auto A, auto B) {
      fx_launch((gemm_f32_wide8_kernel<A(), B(), 3>), P.grid, P.block, 0, s, P.g);
    });
  if (P.np == 2)
    return dispatch_pair<wide8_split_pair>(P.ak, P.bk, "wide8", [&](auto A, auto B) {
      fx_launch((gemm_f32_wide8_kernel<A(), B(), 2>), P.grid, P.block, 0, s, P.g);
    });
  return dispatch_pair<wide8_pair>(P.ak, P.bk, "wide8", [&](auto A, auto B) {
    fx_launch((gemm_f32_wide8_kernel<A(), B(), 0>), P.grid, P.block, 0, s, P.g);
  });
}

}  // namespace fx
