// Device pieces shared by the fused X2Y attention cores (x2y_a2f.hip: frames attend to the action tokens,
// x2y_f2a.hip: tokens attend to the frames): the per-video table of a launch and its lookup, the two tile
// products on v_mfma_f32_32x32x2_f32 (rows x keys over an Hd slice; LDS rows x chunk keys -> Hd column
// tiles), the wave-order sum of partial tiles through LDS and the grid barrier of the one-launch backward
// (the write-through buffer resource `rsrc` of the partials is wave_dev.h's).
#pragma once
#include "fx_common.h"
#include "ops.h"
#include "wave_dev.h"

#include <algorithm>

namespace fx {
namespace x2y_dev {

constexpr int XR = 32;            // a2f: query rows per workgroup
constexpr int XT = 512;           // threads (8 waves)
constexpr int XMAXK = 64;         // a2f: keys per video (the wide variant: FX_X2Y_MAXTOK)
constexpr int FC = 64;            // f2a: keys per chunk
constexpr int FMAXQ = 64;         // f2a: queries per video (the wide variant: FX_X2Y_MAXTOK in blocks of FMAXQ)
constexpr int FX_X2Y_MAXV = 16;   // videos per launch

// ---------------------------------------------------------------- the videos of a launch
struct X2yVideos {
  int yoff[FX_X2Y_MAXV + 1], xoff[FX_X2Y_MAXV + 1];   // first query / key row of each video
  long long aoff[FX_X2Y_MAXV + 1];                    // its (ny_v, nx_v) attention block
  int first[FX_X2Y_MAXV + 1];                         // its first workgroup (a2f) or key chunk (f2a)
};
struct X2yVideo {
  int y0, ny, x0, nx, first;
  long long ao;
};

// r = video v of the table (constant indices only: the argument block stays in SGPRs; filled through the
// reference: returned by value, the selects compile to loads of every video's entries)
__device__ __forceinline__ void x2y_video(const X2yVideos& t, int v, X2yVideo& r) {
#pragma unroll
  for (int i = 0; i < FX_X2Y_MAXV; ++i)
    if (i == v) {
      r.y0 = t.yoff[i];
      r.ny = t.yoff[i + 1] - t.yoff[i];
      r.x0 = t.xoff[i];
      r.nx = t.xoff[i + 1] - t.xoff[i];
      r.ao = t.aoff[i];
      r.first = t.first[i];
    }
}

// r = the video whose workgroups / chunks hold `block`
__device__ __forceinline__ void x2y_block_video(const X2yVideos& t, int nvid, int block, X2yVideo& r) {
  int v = 0;
#pragma unroll
  for (int i = 1; i < FX_X2Y_MAXV; ++i)
    if (i < nvid && block >= t.first[i]) v = i;
  x2y_video(t, v, r);
}

// host: the table of a call, count(ny_v, nx_v) workgroups or chunks per video; returns their total
template <class Count>
inline int x2y_fill_videos(X2yVideos& t, int nvid, const int* yoff, const int* xoff, const long long* aoff, Count count) {
  int n = 0;
  for (int v = 0; v <= nvid; ++v) {
    t.yoff[v] = yoff[v];
    t.xoff[v] = xoff[v];
    t.aoff[v] = aoff[v];
    t.first[v] = n;
    if (v < nvid) n += count(yoff[v + 1] - yoff[v], xoff[v + 1] - xoff[v]);
  }
  for (int v = nvid + 1; v <= FX_X2Y_MAXV; ++v) t.first[v] = n;
  return n;
}
// host: rows of the call's largest video
inline int x2y_max_rows(int nvid, const int* off) {
  int n = 0;
  for (int v = 0; v < nvid; ++v) n = std::max(n, off[v + 1] - off[v]);
  return n;
}

// host: every video of at most maxk keys (the a2f cores' condition)
inline bool a2f_fits(int nvid, const int* xoff, int Hd, int maxk) {
  return nvid >= 1 && nvid <= FX_X2Y_MAXV && Hd % 256 == 0 && Hd <= XT && x2y_max_rows(nvid, xoff) <= maxk;
}

// ---------------------------------------------------------------- tile products
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// 16 consecutive k of one row as MFMA operands, zero for a row outside the tile
__device__ __forceinline__ void frag16(const float* p, bool ok, float (&v)[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 t = ld4(p + 4 * q);
    v[4 * q] = ok ? t.x : 0.f;
    v[4 * q + 1] = ok ? t.y : 0.f;
    v[4 * q + 2] = ok ? t.z : 0.f;
    v[4 * q + 3] = ok ? t.w : 0.f;
  }
}

// acc[c] += A . B_c^T for a 32-row tile and the first nb of NB 32-key blocks over k in [k0, k1) of Hd:
// lane (li, lh) feeds row li (pa) and key li (pb[c]), 16 consecutive k of each 32-deep step, float4 loads
// straight from L2 (the k order inside the sum is free as long as A and B agree); aok / bok: the lane's
// row / key is inside the tile (the pointers are clamped to a valid row)
template <int NB>
__device__ __forceinline__ void tile_qk(const float* pa, bool aok, const float* const (&pb)[NB], const bool (&bok)[NB],
                                        int nb, int k0, int k1, int lh, f32x16 (&acc)[NB]) {
  for (int k = k0; k < k1; k += 32) {
    const int kk = k + 16 * lh;
    float av[16];
    frag16(pa + kk, aok, av);
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      if (c < nb) {
        float bv[16];
        frag16(pb[c] + kk, bok[c], bv);
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[c], 0, 0, 0);
      }
    }
  }
}

// one wave's partial 32 x 32 tile to its slot of `red` (acc register r, lane)
__device__ __forceinline__ void red_store(float* slot, int lane, const f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) slot[r * 64 + lane] = acc[r];
}

// Wave-order sum of the partial tiles in `red`: element e < ne (32 x 32 block e >> 10, acc register, lane)
// is sum_{p < np} red[p stride + e], p ascending (deterministic); out(block, row, col, sum) with (row, col)
// inside the block
template <class F>
__device__ __forceinline__ void wave_sum(const float* red, int stride, int ne, int np, int tid, F&& out) {
  for (int e = tid; e < ne; e += XT) {
    const int r = (e >> 6) & 15, l = e & 63;
    float sum = 0.f;
    for (int p = 0; p < np; ++p) sum += red[p * stride + e];
    out(e >> 10, (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31, sum);
  }
}

// dst[y][n] = mul sum_x S[y][x] Bm[x][n] for y < ny (32-row tiles), the chunk's keys x (K = FC; Bm: the
// chunk's first key row, ld Hd), n < Hd: (row tiles x Hd/32 column tiles) over the 8 waves, A = the LDS tile,
// B = Bm columns (32 lanes read 32 consecutive floats of one key row)
__device__ __forceinline__ void rows_x_keys(const float (*S)[FC + 1], const float* Bm, int ny, int keys, int Hd,
                                            float mul, float* dst, int w, int li, int lh) {
  const int nrb = ny > 32 ? 2 : 1, nct = Hd >> 5;
  for (int t = w; t < nrb * nct; t += 8) {
    const int tr = t / nct, n0 = (t - tr * nct) * 32;
    f32x16 f;
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = 0.f;
#pragma unroll
    for (int kc = 0; kc < FC; kc += 32) {
      float bv[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int key = kc + 16 * lh + s2;
        const float x = Bm[(long long)min(key, keys - 1) * Hd + n0 + li];
        bv[s2] = key < keys ? x : 0.f;
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2)
        f = __builtin_amdgcn_mfma_f32_32x32x2f32(S[tr * 32 + li][kc + 16 * lh + s2], bv[s2], f, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = tr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row < ny) dst[(long long)row * Hd + n0 + li] = mul * f[r];
    }
  }
}

// out[x][n] = mul sum_y L[y][x] Bm[y][n] for the chunk's keys x (rows of out), y < ny (K), n < Hd:
// (2 key tiles x Hd/32 column tiles) over the 8 waves, A = L^T from LDS, B = Bm columns (global); accum: added
// to what the same thread stored for the earlier query blocks (block order, deterministic)
__device__ __forceinline__ void keys_out(const float (*L)[FC + 1], const float* Bm, long long ldb, int ny, int keys,
                                         int Hd, float mul, float* out, int w, int li, int lh, bool accum = false) {
  const int nct = Hd >> 5;
  for (int t = w; t < 2 * nct; t += 8) {
    const int rt = t / nct, n0 = (t - rt * nct) * 32;
    f32x16 f;
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = 0.f;
    for (int k0 = 0; k0 < ny; k0 += 32) {
      float bv[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int y = k0 + 16 * lh + s2;
        const float x = Bm[(long long)min(y, ny - 1) * ldb + n0 + li];
        bv[s2] = y < ny ? x : 0.f;
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int y = k0 + 16 * lh + s2;
        f = __builtin_amdgcn_mfma_f32_32x32x2f32(y < FMAXQ ? L[min(y, FMAXQ - 1)][rt * 32 + li] : 0.f, bv[s2], f, 0, 0,
                                                 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row < keys) {
        float* o = out + (long long)row * Hd + n0 + li;
        *o = accum ? *o + mul * f[r] : mul * f[r];   // (accum: a later query block of the wide variant)
      }
    }
  }
}

// ---------------------------------------------------------------- hand-offs between workgroups
// Grid barrier of the one-launch form (every workgroup co-resident: the grid is capped by the occupancy
// calculator on the host): each workgroup's write-through stores acknowledged (vmcnt 0) before its arrival;
// every workgroup counts its exit, timed out or not, and the last one re-arms the slot.  Bounded spin: a
// workgroup that gives up ORs FX_STATUS_X2Y_TIMEOUT into the caller's status word (read back with the step's
// status, which fails the step and makes FusedAdam skip its update) and goes on -- never a hang
__device__ __forceinline__ void f2a_grid_sync(unsigned* bar, unsigned* status, unsigned spin_max) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned G = gridDim.x;
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned n = 0;
    bool late = false;
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < G) {
      if (++n >= spin_max) {
        late = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (late && status)
      __hip_atomic_fetch_or(status, (unsigned)FX_STATUS_X2Y_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned prev = __hip_atomic_fetch_add(bar + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == G - 1) {   // every workgroup is past the barrier
      __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(bar + 32, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
}

}  // namespace x2y_dev
}  // namespace fx
