// Device helpers shared by the fused layer kernels (mstcn_fused.hip: MS-TCN, mstcn2_fused.hip: MS-TCN++):
// the tile geometry (FR = 32 rows x FN = 256 channels per workgroup, 8 waves x 32 columns, one 32x32 f32
// MFMA accumulator per wave), the activation stage images of the LDS ring, the per-wave weight fragments
// in the packed order of launch_pack_frag, and the row-tile order on the XCDs.
#pragma once
#include "fx_common.h"
#include "wave_dev.h"

namespace fx {
namespace frl_dev {

constexpr int FR = 32;           // rows per workgroup
constexpr int FN = 256;          // channels: N of both GEMMs, K of the second
constexpr int FBK = 32;          // k per stage
constexpr int FT = 512;          // threads: 8 waves x 32 columns
constexpr int AS = FBK + 4;      // LDS row stride of the activation stage images ([row][k], k contiguous)
constexpr int A_IMG = FR * AS;
constexpr int NSL = 3;           // activation ring depth
constexpr int kMaxSeqF = 16;     // ragged videos per launch

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// packed weight fragment of stage st, wave w for this lane: 4 float4 (k = 16 lh + 4 q .. + 3)
__device__ __forceinline__ void load_b(const float* wp, int st, int w, int lane, float4* b) {
  const float* base = wp + ((long long)(st * 8 + w) * 4) * 256 + lane * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) b[q] = ld4(base + q * 256);
}

// A fragments of one 32-deep stage from LDS rows `a` (row stride as): lane (li, lh) takes row li, k 16 lh ..
__device__ __forceinline__ void lds_frag(const float* a, int as, int li, int lh, float4* fa) {
#pragma unroll
  for (int q = 0; q < 4; ++q) fa[q] = ld4(a + li * as + lh * 16 + q * 4);
}

// the 16 MFMAs of one stage from fragments already in registers
__device__ __forceinline__ void mma_frag(const float4* fa, const float4* fb, f32x16& acc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].x, fb[q].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].y, fb[q].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].z, fb[q].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].w, fb[q].w, acc, 0, 0, 0);
  }
}

// Row tile of this workgroup.  Workgroups go to the 8 XCDs round robin by dispatch id, so in plain
// order a tile's neighbours -- whose rows are its conv halo (dilation < FR) or its shifted taps -- sit
// on other XCDs and every tile fetches its halo / taps through its own L2 again.  xcd_runs: XCD x gets
// a contiguous run of tiles; row_perm p > 1 (taps shift by p whole tiles): the runs walk the tiles
// 0, p, 2p, ..., 1, 1 + p, ... so a tile and its shifted taps share the run (the GEMM's block_tile
// does the same for the dilated-conv GEMMs).
__device__ __forceinline__ int frl_tile_id(int xcd_runs, int row_perm) {
  const int id = blockIdx.x;
  if (!xcd_runs) return id;
  const int nt = gridDim.x, q = nt / 8, rr = nt % 8, x8 = id % 8, i8 = id / 8;
  int t = (x8 < rr ? x8 * (q + 1) : rr * (q + 1) + (x8 - rr) * q) + i8;
  if (row_perm > 1) {
    const int per = nt / row_perm;
    t = (t % per) * row_perm + t / per;
  }
  return t;
}

// position of row r inside its video and the video's length: ragged offsets soff[0 .. nsoff] (nsoff > 0),
// else uniform videos of T rows
__device__ __forceinline__ void frl_row_pos(int r, int nsoff, const int* soff, int T, int& rpos, int& rlen) {
  if (nsoff > 0) {
    int start = 0, end = 0x7fffffff;
#pragma unroll
    for (int i = 1; i <= kMaxSeqF; ++i) {
      if (i <= nsoff) {
        const int o = soff[i];
        if (o <= r) start = o;
        else end = min(end, o);
      }
    }
    rpos = r - start;
    rlen = end - start;
  } else {
    rpos = r % T;
    rlen = T;
  }
}

}  // namespace frl_dev
}  // namespace fx
