// The tiled f32 GEMM kernel: 64x64 output tile per 256-thread workgroup (see gemm_dev.h).
#include "gemm_plan.h"

namespace fx {
namespace {

// One pipelined stage for this wave, as ONE basic block (no branches, so the compiler counts
// outstanding loads exactly), in a fixed order pinned by sched_barrier: first the global loads of
// a later stage into set `rn` (they get two MFMA phases to land), then the 32 MFMAs of the
// current slot with each fragment read issued two groups (8 MFMAs, 512 cycles) ahead of its use,
// and the LDS writes of set `rs` (loaded one stage ago) spread over the middle groups.  Two
// accumulators (even / odd fragment groups) keep two independent chains in the matrix core.
template <bool FAST, int AK, int BKd>
__device__ __forceinline__ void stage_body(const Loader<AK, FAST>& la, const Loader<BKd, FAST>& lb, const float* cur,
                                           float* wslot, int kload, const float4* rs_a, const float4* rs_b,
                                           unsigned ms_a, unsigned ms_b, float4* rn_a, float4* rn_b, unsigned& mn_a,
                                           unsigned& mn_b, int wm, int wn, int li, int lh, f32x16& acc0,
                                           f32x16& acc1) {
  using LA = Loader<AK, FAST>;
  using LB = Loader<BKd, FAST>;
  float4 fa[8], fb[8];
  fa[0] = LA::frag(cur, wm * 32, li, lh, 0);
  fb[0] = LB::frag(cur + IMG, wn * 32, li, lh, 0);
  fa[1] = LA::frag(cur, wm * 32, li, lh, 1);
  fb[1] = LB::frag(cur + IMG, wn * 32, li, lh, 1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f32x16& acc = (q & 1) ? acc1 : acc0;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].x, fb[q].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].y, fb[q].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].z, fb[q].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].w, fb[q].w, acc, 0, 0, 0);
    if (q + 2 < 8) {
      fa[q + 2] = LA::frag(cur, wm * 32, li, lh, q + 2);
      fb[q + 2] = LB::frag(cur + IMG, wn * 32, li, lh, q + 2);
    }
    // the next loads' address work runs beside the first MFMA groups, not ahead of them
    if (q == 0) la.load(kload, rn_a, mn_a);
    if (q == 1) lb.load(kload, rn_b, mn_b);
    if (q == 6) la.store(wslot, rs_a, ms_a);   // late: the loads get ~1.7 stages to land
    if (q == 7) lb.store(wslot + IMG, rs_b, ms_b);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The pipelined K loop over stages [kt0, kt1): a 3-slot LDS ring, loads two stages ahead of
// their LDS write.  Out-of-range prefetches are clamped to the last stage (loaded, never used)
// and stores past the end go to a slot nobody reads again, so every iteration is straight-line.
template <bool FAST, int AK, int BKd>
__device__ __forceinline__ void kloop(const Loader<AK, FAST>& la, const Loader<BKd, FAST>& lb, float* lds, int kt0,
                                      int kt1, int wm, int wn, int li, int lh, f32x16& acc0, f32x16& acc1) {
  const int n = kt1 - kt0;
  if (n <= 0) return;
  const int klast = (kt1 - 1) * BK;
  float4 ra0[4], rb0[4], ra1[4], rb1[4];
  unsigned ma0, mb0, ma1, mb1;
  // prologue: stages 0 and 1 into slots 0 and 1, stage 2 in flight in set 0
  la.load(kt0 * BK, ra0, ma0);
  lb.load(kt0 * BK, rb0, mb0);
  la.load(min((kt0 + 1) * BK, klast), ra1, ma1);
  lb.load(min((kt0 + 1) * BK, klast), rb1, mb1);
  la.store(lds, ra0, ma0);
  lb.store(lds + IMG, rb0, mb0);
  la.store(lds + 2 * IMG, ra1, ma1);
  lb.store(lds + 3 * IMG, rb1, mb1);
  la.load(min((kt0 + 2) * BK, klast), ra0, ma0);
  lb.load(min((kt0 + 2) * BK, klast), rb0, mb0);
  __syncthreads();
  // iteration i multiplies slot i%3, writes stage i+2 (held in set i&1) into slot (i+2)%3,
  // and issues the loads of stage i+3 into set (i+1)&1
  int slot = 0;
  auto iter = [&](int i, const float4* rs_a, const float4* rs_b, unsigned ms_a, unsigned ms_b, float4* rn_a,
                  float4* rn_b, unsigned& mn_a, unsigned& mn_b) FX_INLINE {
    const int ws = slot == 0 ? 2 : slot - 1;   // (slot + 2) % 3
    stage_body<FAST, AK, BKd>(la, lb, lds + slot * 2 * IMG, lds + ws * 2 * IMG, min((kt0 + i + 3) * BK, klast), rs_a,
                              rs_b, ms_a, ms_b, rn_a, rn_b, mn_a, mn_b, wm, wn, li, lh, acc0, acc1);
    __syncthreads();
    slot = slot == 2 ? 0 : slot + 1;
  };
  int i = 0;
  for (; i + 1 < n; i += 2) {
    iter(i, ra0, rb0, ma0, mb0, ra1, rb1, ma1, mb1);
    iter(i + 1, ra1, rb1, ma1, mb1, ra0, rb0, ma0, mb0);
  }
  if (i < n) iter(i, ra0, rb0, ma0, mb0, ra1, rb1, ma1, mb1);
}

template <int AK, int BKIND, bool FAST>
__global__ __launch_bounds__(NTHREADS) void gemm_f32_kernel(GemmDev g) {
  __shared__ float lds[NSLOT * 2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  // XCD-aware remap of (x, y) tiles: consecutive remapped ids share an XCD (L2)
  int tx, ty, z;
  block_tile(g, tx, ty, z);
  const int n0 = tx * BN, m0 = ty * BM;
  const int bidx = z / g.split, sk = z - bidx * g.split;
  const int nkt = (g.K + BK - 1) / BK;
  const int kt0 = sk * g.kt_per_split;
  const int kt1 = min(nkt, kt0 + g.kt_per_split);

  Loader<AK, FAST> la;
  Loader<BKIND, FAST> lb;
  la.init(batch_op_a(g.a, g.a_dil_b1, bidx), g.a.ptr + (long long)bidx * g.a.batch_stride, m0, g.M, g.K, tid, g.soff, g.nsoff);
  lb.init(batch_op_b(g.b, g.b_dil_growth, bidx), g.b.ptr + (long long)bidx * g.b.batch_stride, n0, g.N, g.K, tid, g.soff, g.nsoff);

  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc0[i] = 0.f;
    acc1[i] = 0.f;
  }
  FX_STAMP(g, 0);
  kloop<FAST, AK, BKIND>(la, lb, lds, kt0, kt1, wm, wn, li, lh, acc0, acc1);
  FX_STAMP(g, 2);
  f32x16 acc = acc0 + acc1;

  // C/D layout of the 32x32 f32 accumulator: col = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)
  const int col = n0 + wn * 32 + li;
  const int rbase = m0 + wm * 32 + 4 * lh;
  if (g.split > 1) {
    if (col < g.N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + (r & 3) + 8 * (r >> 2);
        if (row < g.M) g.ws[(((long long)bidx * g.split + sk) * g.M + row) * g.N + col] = acc[r];
      }
    }
    if (g.tile_cnt)   // flag: the last word of the LDS ring (free after the k loop's final barrier)
      splitk_finish<BM, BN>(g, bidx, m0, n0, (bidx * g.tiles_y + ty) * g.tiles_x + tx,
                            reinterpret_cast<int*>(&lds[NSLOT * 2 * IMG - 1]));
    return;
  }
  if (col >= g.N) return;
  if (!g.c_last && !g.c_tap_cin && !g.gate && g.beta == 0.f && !g.drop_thr) {
    // common forward epilogue: every read (bias, residual) is issued before the first store,
    // so the 16 loads overlap instead of queueing behind stores they might alias
    const float bv = g.bias ? g.bias[(long long)bidx * g.bias_bs + col] : 0.f;
    float res[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      res[r] = (g.resid && row < g.M) ? g.resid[(long long)bidx * g.resid_bs + (long long)row * g.ld_resid + col]
                                      : 0.f;
    }
    float* cb = g.c + (long long)bidx * g.c_bs + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      float v = g.alpha * acc[r] + bv;
      if (g.relu == 2) v = fmaxf(v, 0.f);
      v += res[r];
      if (g.relu == 1) v = fmaxf(v, 0.f);
      if (row < g.M) cb[(long long)row * g.ldc] = v;
    }
  } else if (g.beta != 0.f) {
    // accumulating (dW into param.grad): load the 16 old values before the first store
    float cold[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) cold[r] = *epilogue_ptr(g, bidx, min(rbase + (r & 3) + 8 * (r >> 2), g.M - 1), col);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      if (row < g.M) epilogue_store(g, bidx, row, col, acc[r], true, cold[r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      if (row < g.M) epilogue_store(g, bidx, row, col, acc[r]);
    }
  }
  FX_STAMP(g, 3);
}

}  // namespace

int launch_tiled(const GemmPlan& P, hipStream_t s) {
  const int bk = gen_kind(P.bk);
  if (P.fast)
    return dispatch_pair<tiled_fast_pair>(P.ak, bk, "tiled", [&](auto A, auto B) {
      fx_launch((gemm_f32_kernel<A(), B(), true>), P.grid, P.block, 0, s, P.g);
    });
  return dispatch_pair<tiled_generic_pair>(P.ak, bk, "tiled", [&](auto A, auto B) {
    fx_launch((gemm_f32_kernel<A(), B(), false>), P.grid, P.block, 0, s, P.g);
  });
}

}  // namespace fx
