#include "gemm_plan.h"

namespace fx {
namespace {

// ---------------------------------------------------------------- direct kernel (small shapes)
// Token-level (M = Nact = 32) projections, per-head attention products and their weight
// gradients are far too small for the 64x64 LDS-tiled kernel: its per-tile cost is latency
// (prologue loads, a 1 us MFMA phase per 64-deep stage, the epilogue), so a handful of tiles
// walking K serially takes 10-30 us.  Here each wave owns one 32x32 output tile over a strided
// set of 32-deep k chunks and loads its MFMA fragments straight from global memory (L2): a lane
// takes 16 CONSECUTIVE k of a chunk (the k order inside an MFMA chain is free as long as A and B
// agree), so row-major operands are float4 loads and column-major ones are coalesced across
// lanes.  The waves of a block split K of the same tile and are summed through LDS in wave
// order; optional cross-block split-K goes through workspace slabs + splitk_finish.

template <int KIND>
__device__ __forceinline__ void dload(const fx_operand& o, const float* base, int r, int R, int k0, int K, bool vec,
                                      float* v, const SeqOff& soff, int nsoff) {
  if (KIND == ROWS) {
    if (vec && r < R && k0 + 16 <= K) {
      const float* p = base + (long long)r * o.ld + k0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(p + 4 * q);
        v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
      }
      return;
    }
    // edge chunk: clamped, unconditional loads (all 16 in flight at once), zeroed by select
    const int rc = min(r, R - 1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float x = base[(long long)rc * o.ld + min(k0 + j, K - 1)];
      v[j] = (r < R && k0 + j < K) ? x : 0.f;
    }
  } else if (KIND == COLS) {
    // clamped, unconditional loads so the compiler issues all 16 before the first wait (the ones
    // column is a virtual operand column: its row index is clamped too and the value replaced)
    const bool ones = o.ones_col && r == o.ones_col - 1;
    const int rc = max(min(r, o.ones_col ? o.ones_col - 2 : R - 1), 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float x = base[(long long)min(k0 + j, K - 1) * o.ld + rc];
      v[j] = (r < R && k0 + j < K) ? (ones ? 1.f : x) : 0.f;
    }
  } else {  // ROWS_GEN
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (r < R && k0 + j < K) ? fetch_rm(o, base, r, k0 + j, soff, nsoff) : 0.f;
  }
}

__device__ __forceinline__ void direct_finish(const GemmDev& g, int bidx, int sk, int row, int col, float v) {
  if (row >= g.M || col >= g.N) return;
  if (g.split > 1)
    g.ws[(((long long)bidx * g.split + sk) * g.M + row) * g.N + col] = v;
  else
    epilogue_store(g, bidx, row, col, v);
}

template <int AK, int BKd>
__device__ __forceinline__ void direct_body(const GemmDev& g, int bx, int by, int z, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = bx * 32, m0 = by * 32;
  const int bidx = z / g.split, sk = z - bidx * g.split;
  const int nch = (g.K + DCH - 1) / DCH;
  const int c0 = sk * g.kt_per_split, c1 = min(nch, c0 + g.kt_per_split);
  const float* pa = g.a.ptr + (long long)bidx * g.a.batch_stride;
  const float* pb = g.b.ptr + (long long)bidx * g.b.batch_stride;
  const int ra = m0 + li, rb = n0 + li, ko = lh * 16;
  const bool av = g.a_vec, bv = g.b_vec;

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float a0[16], b0[16], a1[16], b1[16];
  int c = c0 + w;
  if (c < c1) {
    dload<AK>(g.a, pa, ra, g.M, c * DCH + ko, g.K, av, a0, g.soff, g.nsoff);
    dload<BKd>(g.b, pb, rb, g.N, c * DCH + ko, g.K, bv, b0, g.soff, g.nsoff);
  }
  for (; c < c1; c += 2 * nw) {
    const int cn = c + nw;
    if (cn < c1) {
      dload<AK>(g.a, pa, ra, g.M, cn * DCH + ko, g.K, av, a1, g.soff, g.nsoff);
      dload<BKd>(g.b, pb, rb, g.N, cn * DCH + ko, g.K, bv, b1, g.soff, g.nsoff);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc, 0, 0, 0);
    const int cnn = cn + nw;
    if (cnn < c1) {
      dload<AK>(g.a, pa, ra, g.M, cnn * DCH + ko, g.K, av, a0, g.soff, g.nsoff);
      dload<BKd>(g.b, pb, rb, g.N, cnn * DCH + ko, g.K, bv, b0, g.soff, g.nsoff);
    }
    if (cn < c1) {
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc, 0, 0, 0);
    }
  }

  if (nw > 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    for (int e = tid; e < 1024; e += nw * 64) {
      const int r = e >> 6, l = e & 63;
      float v = 0.f;
      for (int q = 0; q < nw; ++q) v += red[(q * 16 + r) * 64 + l];
      direct_finish(g, bidx, sk, m0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n0 + (l & 31), v);
    }
  } else if (g.split > 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) direct_finish(g, bidx, sk, m0 + (r & 3) + 8 * (r >> 2) + 4 * lh, n0 + li, acc[r]);
  } else if (g.beta != 0.f) {
    // accumulate into C (e.g. K = 64 dW GEMMs into param.grad): all 16 old values are loaded
    // before the first store; element by element each store would hold back the next load
    float cold[16];
    const int col = min(n0 + li, g.N - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) cold[r] = *epilogue_ptr(g, bidx, min(m0 + (r & 3) + 8 * (r >> 2) + 4 * lh, g.M - 1), col);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row < g.M && n0 + li < g.N) epilogue_store(g, bidx, row, n0 + li, acc[r], true, cold[r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) direct_finish(g, bidx, sk, m0 + (r & 3) + 8 * (r >> 2) + 4 * lh, n0 + li, acc[r]);
  }
  if (g.split > 1 && g.tile_cnt)
    splitk_finish<32, 32>(g, bidx, m0, n0, (bidx * g.tiles_y + by) * g.tiles_x + bx,
                          reinterpret_cast<int*>(&red[DMAXW * 16 * 64]));
}

template <int AK, int BKd>
__global__ __launch_bounds__(DMAXW * 64) void gemm_direct_kernel(GemmDev g) {
  __shared__ float red[DMAXW * 16 * 64 + 1];   // wave partials + the split-K "last block" flag
  direct_body<AK, BKd>(g, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

// Several independent small GEMMs in ONE launch (e.g. the dW/db and dX GEMMs of one linear layer, both
// reading the same dY): the flat block index picks the problem (block-uniform), each problem keeps
// its own grid, operand kinds, split and epilogue.  Saves a launch (~2.7 us back to back) per member.
__device__ __forceinline__ void direct_dispatch(const GemmDev& g, int kinds, int local, float* red) {
  const int txy = g.tiles_x * g.tiles_y;
  const int z = local / txy, r = local - z * txy, by = r / g.tiles_x, bx = r - by * g.tiles_x;
  switch (kinds) {
    case ROWS * 8 + ROWS: direct_body<ROWS, ROWS>(g, bx, by, z, red); break;
    case ROWS * 8 + COLS: direct_body<ROWS, COLS>(g, bx, by, z, red); break;
    case ROWS_GEN * 8 + ROWS: direct_body<ROWS_GEN, ROWS>(g, bx, by, z, red); break;
    case ROWS_GEN * 8 + COLS: direct_body<ROWS_GEN, COLS>(g, bx, by, z, red); break;
    case COLS * 8 + ROWS: direct_body<COLS, ROWS>(g, bx, by, z, red); break;
    case COLS * 8 + COLS: direct_body<COLS, COLS>(g, bx, by, z, red); break;
    default: break;
  }
}

__global__ __launch_bounds__(DMAXW * 64) void gemm_direct_group_kernel(GemmGroup G) {
  __shared__ float red[DMAXW * 16 * 64 + 1];
  const int id = blockIdx.x;
  // constant member indices only (a runtime index into the kernel argument would copy it to scratch)
  if (id < G.start[1]) direct_dispatch(G.g[0], G.kinds[0], id, red);
  else if (id < G.start[2]) direct_dispatch(G.g[1], G.kinds[1], id - G.start[1], red);
  else if (id < G.start[3]) direct_dispatch(G.g[2], G.kinds[2], id - G.start[2], red);
  else direct_dispatch(G.g[3], G.kinds[3], id - G.start[3], red);
}

}  // namespace

int launch_direct(const GemmPlan& P, hipStream_t s) {
  return dispatch_pair<direct_pair>(gen_kind(P.ak), P.bk, "direct", [&](auto A, auto B) {
    fx_launch((gemm_direct_kernel<A(), B()>), P.grid, P.block, 0, s, P.g);
  });
}

void launch_direct_group(const GemmGroup& G, int blocks, unsigned threads, hipStream_t s) {
  fx_launch(gemm_direct_group_kernel, dim3(blocks), dim3(threads), 0, s, G);
}

}  // namespace fx
