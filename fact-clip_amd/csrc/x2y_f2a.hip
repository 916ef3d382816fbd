// X2Y attention core for a LONG key side (the f2a map): X = frames (nx up to T keys), Y = the action tokens
// (ny <= 64 queries per video), Hd = 512:
//   chunk kernel, one workgroup per 64 keys of a video: S = scale yq . xk_chunk^T (ny x 64, the Hd-deep
//   sum split over the waves), logit written, chunk row max m_c and sum l_c = sum exp(S - m_c), the
//   partial F_c = exp(S - m_c) . xv_chunk (ny x Hd) to a workspace slab;
//   merge kernel, one workgroup per (video, query row): M = max_c m_c, L = sum_c l_c e^(m_c - M),
//   feat = sum_c e^(m_c - M) F_c / L in chunk order (deterministic), attn = exp(logit - M) / L.
// Algorithmic bytes per video: xk, xv (2 nx Hd floats) + logit / attn (2 ny nx) + feat; the slabs add
// 2 ny Hd floats per 64 keys (write + read), 1/32 of the key bytes at ny = 32.
// Also here: the dispatch between the a2f and f2a cores (x2y_core_pick).
#include "x2y_dev.h"

namespace fx {
namespace {
using namespace x2y_dev;

constexpr int FWMAXQ = 320;        // queries per video, wide variant
static_assert(FWMAXQ == FX_X2Y_MAXTOK, "wide f2a core: query blocks of 64 up to FX_X2Y_MAXTOK");

struct F2aArgs {
  const float* yq;      // (Ny, Hd)
  const float* xk;      // (Nx, Hd)
  const float* xv;      // (Nx, Hd)
  float* logit;         // per video (ny_v, nx_v) at aoff[v]
  float* attn;
  float* feat;          // (Ny, Hd)
  float* part;          // (chunks, qrows, Hd) partial F_c
  float* stats;         // (chunks, qrows, 2): m_c, l_c
  int Hd, nvid;
  int qrows;            // slab rows per chunk: FMAXQ, or 64 x the query blocks of the widest video (wide variant)
  float scale;
  X2yVideos vid;        // first[]: first chunk of each video
};

// the key chunk of this workgroup (grid x = the call's chunks)
struct F2aChunk {
  int y0, ny, x0, nx, c0;   // the video: first query / key row, their counts, its first chunk
  long long ao;
  int chunk, k0c, keys;     // the chunk, its first key (video-local), its keys
};
__device__ __forceinline__ F2aChunk f2a_chunk(const X2yVideos& t, int nvid) {
  X2yVideo vd{};
  x2y_block_video(t, nvid, blockIdx.x, vd);
  const int k0c = ((int)blockIdx.x - vd.first) * FC;
  return {vd.y0, vd.ny, vd.x0, vd.nx, vd.first, vd.ao, (int)blockIdx.x, k0c, min(FC, vd.nx - k0c)};
}

// T = A . B_c^T over Hd for ny <= 64 rows of A (ld lda) and the chunk's keys (Bc: its first key row, ld Hd):
// (query block rb, key block cb) blocks of 32 x 32, the waves of a block split Hd (tile_qk), their partial
// tiles summed through `red` in wave order; out(row, col, sum) for every element of the blocks
template <class F>
__device__ __forceinline__ void f2a_rows_qk(const float* A, long long lda, const float* Bc, int ny, int keys, int Hd,
                                            float* red, F&& out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int nrb = ny > 32 ? 2 : 1;                      // 32-row query blocks
  const int nblk = 2 * nrb;                             // output blocks (query block, key block)
  const int wpb = 8 / nblk;                             // waves per block (4 or 2)
  const int blk = w % nblk, kpart = w / nblk;
  const int q = (blk >> 1) * 32 + li, key = (blk & 1) * 32 + li;
  const float* pb[1] = {Bc + (long long)min(key, keys - 1) * Hd};
  const bool bok[1] = {key < keys};
  f32x16 acc[1];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
  const int kw = Hd / wpb;
  tile_qk<1>(A + (long long)min(q, ny - 1) * lda, q < ny, pb, bok, 1, kpart * kw, (kpart + 1) * kw, lh, acc);
  red_store(red + w * 1024, lane, acc[0]);
  __syncthreads();
  wave_sum(red, nblk * 1024, nblk * 1024, wpb, tid,
           [&](int b, int row, int col, float sum) { out((b >> 1) * 32 + row, (b & 1) * 32 + col, sum); });
  __syncthreads();
}

// WIDE: up to FWMAXQ queries per video -- the queries are independent, so the 64-query blocks are grid y
// (a loop over them inside the chunk's workgroup measured slower than the grouped GEMMs from 200 queries:
// 128 workgroups of five blocks each leave half the device idle), each block exactly the pass below at its
// row offset of the slab, the xk / xv chunk shared through L2; !WIDE is the <= 64-query kernel
// (one block, FMAXQ slab rows)
template <bool WIDE>
__global__ __launch_bounds__(XT) void x2y_f2a_chunk_kernel(F2aArgs a) {
  __shared__ float red[8 * 16 * 64];
  __shared__ float S[FMAXQ][FC + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const F2aChunk c = f2a_chunk(a.vid, a.nvid);
  const int Hd = a.Hd, keys = c.keys;
  const int qrows = WIDE ? a.qrows : FMAXQ;
  const int q0 = WIDE ? (int)blockIdx.y * FMAXQ : 0;    // first query of the block (video-local)
  if (WIDE && q0 >= c.ny) return;                       // (uniform: a narrower video of the call)
  const int ny = WIDE ? min(FMAXQ, c.ny - q0) : c.ny;   // queries of the block

  // ---- 1. S = scale yq . xk_chunk^T ----
  f2a_rows_qk(a.yq + (long long)(c.y0 + q0) * Hd, Hd, a.xk + (long long)(c.x0 + c.k0c) * Hd, ny, keys, Hd, red,
              [&](int row, int col, float sum) { S[row][col] = a.scale * sum; });

  // ---- 2. logit out; chunk row max / sum; S <- exp(S - m) (0 outside the chunk's keys) ----
  {
    // 8 threads per query row (64 rows), 8 keys each
    const int row = tid >> 3, c8 = tid & 7;
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c8 + 8 * j;
      if (col < keys) m = fmaxf(m, S[row][col]);
    }
#pragma unroll
    for (int o = 4; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 8));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c8 + 8 * j;
      const float t = S[row][col];
      if (row < ny && col < keys) a.logit[c.ao + (long long)(q0 + row) * c.nx + c.k0c + col] = t;
      const float e = col < keys ? __expf(t - m) : 0.f;
      sum += e;
      S[row][col] = e;   // (read and rewritten by the same thread)
    }
#pragma unroll
    for (int o = 4; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 8);
    if (c8 == 0 && row < ny) {
      a.stats[((long long)c.chunk * qrows + q0 + row) * 2] = m;
      a.stats[((long long)c.chunk * qrows + q0 + row) * 2 + 1] = sum;
    }
  }
  __syncthreads();

  // ---- 3. F_c = S . xv_chunk ----
  rows_x_keys(S, a.xv + (long long)(c.x0 + c.k0c) * Hd, ny, keys, Hd, 1.f,
              a.part + ((long long)c.chunk * qrows + q0) * Hd, w, li, lh);
}

// one workgroup per (video, query row)
template <bool WIDE>
__global__ __launch_bounds__(XT) void x2y_f2a_merge_kernel(F2aArgs a) {
  __shared__ float wgt[1024];
  __shared__ float ML[2];
  const int tid = threadIdx.x;
  const int qrows = WIDE ? a.qrows : FMAXQ;
  const int row = blockIdx.x;
  X2yVideo vd{};
  x2y_video(a.vid, blockIdx.y, vd);
  const int y0 = vd.y0, ny = vd.ny, nx = vd.nx, c0 = vd.first;
  const long long ao = vd.ao;
  if (row >= ny || nx == 0) return;
  const int nch = (nx + FC - 1) / FC;
  if (tid < 64) {
    // M and L over the video's chunks, one wave, fixed order per lane then a fixed shuffle tree
    float m = -3.0e38f;
    for (int c = tid; c < nch; c += 64) m = fmaxf(m, a.stats[((long long)(c0 + c) * qrows + row) * 2]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float l = 0.f;
    for (int c = tid; c < nch; c += 64) {
      const float* st = a.stats + ((long long)(c0 + c) * qrows + row) * 2;
      l += st[1] * __expf(st[0] - m);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) l += __shfl_xor(l, o, 64);
    if (tid == 0) {
      ML[0] = m;
      ML[1] = l;
    }
  }
  __syncthreads();
  const float M = ML[0], invL = 1.f / ML[1];
  for (int c = tid; c < nch; c += XT) wgt[c] = __expf(a.stats[((long long)(c0 + c) * qrows + row) * 2] - M) * invL;
  __syncthreads();
  for (int n = tid; n < a.Hd; n += XT) {
    float acc = 0.f;
    for (int c = 0; c < nch; ++c) acc += wgt[c] * a.part[((long long)(c0 + c) * qrows + row) * a.Hd + n];
    a.feat[(long long)(y0 + row) * a.Hd + n] = acc;
  }
  const long long o = ao + (long long)row * nx;
  for (int x = tid; x < nx; x += XT) a.attn[o + x] = __expf(a.logit[o + x] - M) * invL;
}

// ---------------------------------------------------------------- long key side, backward
// Input-gradient side of the f2a core (frames = keys, tokens = queries), per 64-key chunk:
//   pass 1: dP = dfeat . xv_c^T (+ dattn) -> dL (temporarily), the chunk's share of rowdot = sum_x attn dP,
//           dxv_c = attn_c^T . dfeat (complete: a key row belongs to one chunk);
//   pass 2: rowdot = sum of the video's chunk shares (fixed order), dlogit = attn (dP - rowdot) (+ direct
//           dlogit) -> dL, dxk_c = scale dlogit_c^T . yq (complete), dyq partial = scale dlogit_c . xk_c;
//   merge:  dyq = sum_c partial (chunk order).
// The phases below work on one block of <= 64 queries [q0, q0 + ny) of the chunk's video: the narrow kernel
// calls each once (q0 = 0, slabs of FMAXQ rows), the wide kernel inside its loops over the query blocks.
struct F2aBwdArgs {
  const float* dfeat;   // (Ny, Hd) rows, ld ldf
  long long ldf;
  const float* attn;    // per video (ny_v, nx_v) at aoff[v]
  const float* dattn;   // nullable, same layout
  const float* dl_in;   // nullable, same layout
  const float* xv;      // (Nx, Hd)
  const float* xk;
  const float* yq;      // (Ny, Hd)
  float* dL;            // per video (ny_v, nx_v) at aoff[v]
  float* dxv;           // (Nx, Hd)
  float* dxk;
  float* dyq;           // (Ny, Hd)
  float* part;          // (chunks, qrows, Hd)
  float* stats;         // (chunks, qrows, 2)
  int qrows;            // slab rows per chunk: FMAXQ, or 64 x the query blocks of the widest video (wide variant)
  unsigned* bar;        // one-launch form: {arrivals, ..., exits at +32} of the stream's counter pool
  unsigned* status;     // caller's status word (nullable): FX_STATUS_X2Y_TIMEOUT when the barrier gives up
  unsigned spin_max;    // barrier polls before a workgroup gives up
  int Hd, nvid;
  float scale;
  X2yVideos vid;        // first[]: first chunk of each video
};
typedef float F2aTile[FC + 1];   // a row of an LDS tile (rows = the block's queries, cols = the chunk's keys)

// the block's attn (and, with_dp, its dP from dL) into LDS, zero outside (queries < ny, keys < keys)
__device__ __forceinline__ void f2ab_load(const F2aBwdArgs& a, const F2aChunk& c, F2aTile* Pa, F2aTile* S, int q0,
                                          int ny, bool with_dp) {
  for (int e = threadIdx.x; e < FMAXQ * FC; e += XT) {
    const int y = e / FC, x = e - y * FC;
    const bool ok = y < ny && x < c.keys;
    const long long o = c.ao + (long long)(q0 + y) * c.nx + c.k0c + x;
    Pa[y][x] = ok ? a.attn[o] : 0.f;
    if (with_dp) S[y][x] = ok ? a.dL[o] : 0.f;
  }
}

// dP = dfeat . xv_c^T (+ dattn) -> S (dp_out: and dL, where pass 2 reads it back), the chunk's share of the
// row dots -> stats (PASS 3: written through for the other workgroups), dxv_c (+)= attn_c^T . dfeat
template <int PASS>
__device__ __forceinline__ void f2ab_dp_phase(const F2aBwdArgs& a, const F2aChunk& c, float* red, F2aTile* S,
                                              F2aTile* Pa, int q0, int ny, int qrows, bool accum, bool dp_out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int Hd = a.Hd, keys = c.keys;
  f2a_rows_qk(a.dfeat + (long long)(c.y0 + q0) * a.ldf, a.ldf, a.xv + (long long)(c.x0 + c.k0c) * Hd, ny, keys, Hd, red,
              [&](int row, int col, float sum) {
                if (a.dattn && row < ny && col < keys) sum += a.dattn[c.ao + (long long)(q0 + row) * c.nx + c.k0c + col];
                S[row][col] = sum;
              });
  {
    const int row = tid >> 3, c8 = tid & 7;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c8 + 8 * j;
      if (row < ny && col < keys) {
        if (dp_out) a.dL[c.ao + (long long)(q0 + row) * c.nx + c.k0c + col] = S[row][col];
        part += Pa[row][col] * S[row][col];
      }
    }
#pragma unroll
    for (int o = 4; o >= 1; o >>= 1) part += __shfl_xor(part, o, 8);
    if (c8 == 0 && row < ny) {
      const long long si = ((long long)c.chunk * qrows + q0 + row) * 2;
      if (PASS == 3) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(part), rsrc(a.stats), (int)(si * 4), 0, 16);
      else a.stats[si] = part;
    }
  }
  keys_out(Pa, a.dfeat + (long long)(c.y0 + q0) * a.ldf, a.ldf, ny, keys, Hd, 1.f,
           a.dxv + (long long)(c.x0 + c.k0c) * Hd, w, li, lh, accum);
}

// rdot = the block's row dots: the shares of the video's chunks in chunk order (PASS 3: read write-through,
// after the grid barrier)
template <int PASS>
__device__ __forceinline__ void f2ab_rowdot(const F2aBwdArgs& a, const F2aChunk& c, float* rdot, int q0, int ny,
                                            int qrows) {
  const int tid = threadIdx.x;
  if (tid >= FMAXQ) return;
  const int nch = (c.nx + FC - 1) / FC;
  float sum = 0.f;
  if (tid < ny)
    for (int ch = 0; ch < nch; ++ch) {
      const long long si = ((long long)(c.c0 + ch) * qrows + q0 + tid) * 2;
      if (PASS == 3) sum += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc(a.stats), (int)(si * 4), 0, 16));
      else sum += a.stats[si];
    }
  rdot[tid] = sum;
}

// dlogit = attn (dP - rowdot) (+ direct) -> dL and S, dxk_c (+)= scale dlogit_c^T . yq, the dyq partial
// scale dlogit_c . xk_c -> the chunk's slab
__device__ __forceinline__ void f2ab_dlogit_phase(const F2aBwdArgs& a, const F2aChunk& c, F2aTile* S, const F2aTile* Pa,
                                                  const float* rdot, int q0, int ny, int qrows, bool accum) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int Hd = a.Hd, keys = c.keys;
  for (int e = tid; e < FMAXQ * FC; e += XT) {
    const int y = e / FC, x = e - y * FC;
    float d = 0.f;
    if (y < ny && x < keys) {
      const long long o = c.ao + (long long)(q0 + y) * c.nx + c.k0c + x;
      d = Pa[y][x] * (S[y][x] - rdot[y]);
      if (a.dl_in) d += a.dl_in[o];
      a.dL[o] = d;
    }
    S[y][x] = d;   // (read and rewritten by the same thread)
  }
  __syncthreads();
  keys_out(S, a.yq + (long long)(c.y0 + q0) * Hd, Hd, ny, keys, Hd, a.scale, a.dxk + (long long)(c.x0 + c.k0c) * Hd, w,
           li, lh, accum);
  rows_x_keys(S, a.xk + (long long)(c.x0 + c.k0c) * Hd, ny, keys, Hd, a.scale,
              a.part + ((long long)c.chunk * qrows + q0) * Hd, w, li, lh);
}

// PASS 1: dP, its row-dot partials, dxv; PASS 2: dlogit, dxk, the dyq partials (reading dP back);
// PASS 3: both in one launch, dP kept in LDS, a grid barrier for the row dots in between
template <int PASS>
__global__ __launch_bounds__(XT) void x2y_f2a_bwd_kernel(F2aBwdArgs a) {
  __shared__ float red[8 * 16 * 64];
  __shared__ float S[FMAXQ][FC + 1];    // dP, then dlogit (rows = queries, cols = the chunk's keys)
  __shared__ float Pa[FMAXQ][FC + 1];   // attn of the chunk
  __shared__ float rdot[FMAXQ];
  const F2aChunk c = f2a_chunk(a.vid, a.nvid);
  f2ab_load(a, c, Pa, S, 0, c.ny, PASS == 2);
  if (PASS == 2) f2ab_rowdot<2>(a, c, rdot, 0, c.ny, FMAXQ);
  __syncthreads();
  if (PASS != 2) f2ab_dp_phase<PASS>(a, c, red, S, Pa, 0, c.ny, FMAXQ, false, PASS == 1);
  if (PASS == 3) {
    // every chunk's row-dot partial written through: the row sums of this video's chunks
    f2a_grid_sync(a.bar, a.status, a.spin_max);
    f2ab_rowdot<3>(a, c, rdot, 0, c.ny, FMAXQ);
    __syncthreads();
  }
  if (PASS != 1) f2ab_dlogit_phase(a, c, S, Pa, rdot, 0, c.ny, FMAXQ, false);
}

// The wide variant (65 .. FWMAXQ queries per video): the chunk's workgroup loops over 64-query blocks, the
// grid stays one workgroup per key chunk.  dP of every block goes through dL in all three forms (the LDS
// tiles hold one block), so PASS 3 is pass 1 over every block, the grid barrier, pass 2 over every block;
// dxv_c / dxk_c accumulate over the blocks in block order (keys_out accum: each element by one thread).
// (A kernel of its own: one instantiation for both would cost the narrow kernel the wide one's registers.)
template <int PASS>
__global__ __launch_bounds__(XT) void x2y_f2a_bwd_wide_kernel(F2aBwdArgs a) {
  __shared__ float red[8 * 16 * 64];
  __shared__ float S[FMAXQ][FC + 1];    // dP, then dlogit of the query block
  __shared__ float Pa[FMAXQ][FC + 1];   // attn of the query block
  __shared__ float rdot[FMAXQ];
  const F2aChunk c = f2a_chunk(a.vid, a.nvid);
  const int qrows = a.qrows;
  const int nqb = (c.ny + FMAXQ - 1) / FMAXQ;
  if (PASS != 2)
    for (int qb = 0; qb < nqb; ++qb) {
      const int q0 = qb * FMAXQ, ny = min(FMAXQ, c.ny - q0);
      f2ab_load(a, c, Pa, S, q0, ny, false);   // (read after the barriers of the dP product)
      f2ab_dp_phase<PASS>(a, c, red, S, Pa, q0, ny, qrows, qb > 0, true);
      __syncthreads();   // (Pa, S and red are rewritten by the next query block)
    }
  // every chunk's row-dot partials written through (and this workgroup's dP stores acknowledged)
  if (PASS == 3) f2a_grid_sync(a.bar, a.status, a.spin_max);
  if (PASS != 1)
    for (int qb = 0; qb < nqb; ++qb) {
      const int q0 = qb * FMAXQ, ny = min(FMAXQ, c.ny - q0);
      f2ab_load(a, c, Pa, S, q0, ny, true);
      f2ab_rowdot<PASS>(a, c, rdot, q0, ny, qrows);
      __syncthreads();
      f2ab_dlogit_phase(a, c, S, Pa, rdot, q0, ny, qrows, qb > 0);
      __syncthreads();   // (Pa, S and rdot are rewritten by the next query block)
    }
}

// dyq = sum of the chunk partials in chunk order, one workgroup per (query row, video)
template <bool WIDE>
__global__ __launch_bounds__(XT) void x2y_f2a_bwd_merge_kernel(F2aBwdArgs a) {
  const int qrows = WIDE ? a.qrows : FMAXQ;
  const int row = blockIdx.x;
  X2yVideo vd{};
  x2y_video(a.vid, blockIdx.y, vd);
  if (row >= vd.ny) return;
  const int nch = (vd.nx + FC - 1) / FC;
  for (int n = threadIdx.x; n < a.Hd; n += XT) {
    float acc = 0.f;
    for (int c = 0; c < nch; ++c) acc += a.part[((long long)(vd.first + c) * qrows + row) * a.Hd + n];
    a.dyq[(long long)(vd.y0 + row) * a.Hd + n] = acc;
  }
}

// every video of at most maxq queries and 1024 key chunks (the f2a cores' condition)
bool f2a_fits(int nvid, const int* xoff, const int* yoff, int Hd, int maxq) {
  if (nvid < 1 || nvid > FX_X2Y_MAXV || Hd % 256 != 0 || Hd > XT) return false;
  if (x2y_max_rows(nvid, yoff) > maxq) return false;
  if ((x2y_max_rows(nvid, xoff) + FC - 1) / FC > 1024) return false;     // merge weights in LDS
  return x2y_f2a_chunks(nvid, xoff) > 0;
}

// slab rows per chunk of a call: FMAXQ, or 64 x the query blocks of the widest video
int f2a_qrows(int nvid, const int* yoff) {
  const int maxq = x2y_max_rows(nvid, yoff);
  // (a call past the wide core's queries never reaches the kernels: sized as one block)
  return maxq <= FMAXQ || maxq > FWMAXQ ? FMAXQ : (maxq + FMAXQ - 1) / FMAXQ * FMAXQ;
}

// the table, slab rows and workspace split of a call (Args: F2aArgs or F2aBwdArgs); returns its chunks
template <class Args>
int f2a_prepare(Args& a, int nvid, const int* yoff, const int* xoff, const long long* aoff, int Hd, float* ws) {
  const int nch = x2y_fill_videos(a.vid, nvid, yoff, xoff, aoff, [](int, int nx) { return (nx + FC - 1) / FC; });
  a.Hd = Hd;
  a.nvid = nvid;
  a.qrows = f2a_qrows(nvid, yoff);
  a.part = ws;
  a.stats = ws + (long long)nch * a.qrows * Hd;
  return nch;
}

// the backward's launches: one launch when every chunk's workgroup can be resident at once (the grid barrier
// waits for all of them): the occupancy calculator's bound for this kernel on this device (CU count x
// workgroups per CU); FX_X2Y_F2A_ONE=0 keeps the two launches (A/B).  The wide variant has the same grid
// (one workgroup per key chunk, each looping over its query blocks), so the same kind of bound
template <bool WIDE>
void f2a_bwd_launches(F2aBwdArgs& a, int nch, int maxq, hipStream_t s) {
  const auto pass1 = WIDE ? x2y_f2a_bwd_wide_kernel<1> : x2y_f2a_bwd_kernel<1>;
  const auto pass2 = WIDE ? x2y_f2a_bwd_wide_kernel<2> : x2y_f2a_bwd_kernel<2>;
  const auto pass3 = WIDE ? x2y_f2a_bwd_wide_kernel<3> : x2y_f2a_bwd_kernel<3>;
  const int resident = coresident_blocks((const void*)pass3, XT, 0);
  a.bar = (knobs().x2y_f2a_one && nch <= resident) ? arrival_counters(s) : nullptr;
  if (a.bar) {
    fx_launch(pass3, dim3(nch), dim3(XT), 0, s, a);
  } else {
    fx_launch(pass1, dim3(nch), dim3(XT), 0, s, a);
    fx_launch(pass2, dim3(nch), dim3(XT), 0, s, a);
  }
  fx_launch(x2y_f2a_bwd_merge_kernel<WIDE>, dim3(maxq, a.nvid), dim3(XT), 0, s, a);
}

}  // namespace

bool x2y_f2a_fusable(int nvid, const int* xoff, const int* yoff, int Hd) {
  return f2a_fits(nvid, xoff, yoff, Hd, FMAXQ);
}

// THE dispatch of fx_x2y_fwd / fx_x2y_bwd / fx_x2y_workspace_floats (alignment and knobs aside): the
// <= 64-row cores first, exactly as before the wide variants existed (a segment-level f2a call of 65 .. 320
// segments and <= 64 tokens stays on the f2a core), then the wide a2f core, then the wide f2a core.  The
// wide cores are taken at frame level only (the level as fx_prof tells the calls apart: max(Nx, Ny) >=
// 1024 rows in the call, which includes the shipped yaml's ~3400 segments): in segment-level calls both
// measured slower than the grouped GEMMs (profiles/x2y_tokens.json: 2 x 100 query rows are 8 workgroups
// of the a2f core, 2 x 400 keys 14 of the f2a core), and such a shape class keeps the grouped path
constexpr int kFrameLevelRows = 1024;
int x2y_core_pick(int nvid, const int* xoff, const int* yoff, int Hd) {
  if (a2f_fits(nvid, xoff, Hd, XMAXK)) return FX_X2Y_CORE_A2F;
  if (f2a_fits(nvid, xoff, yoff, Hd, FMAXQ)) return FX_X2Y_CORE_F2A;
  if (std::max(xoff[nvid], yoff[nvid]) < kFrameLevelRows) return FX_X2Y_CORE_NONE;
  if (a2f_fits(nvid, xoff, Hd, FX_X2Y_MAXTOK)) return FX_X2Y_CORE_A2F_WIDE;
  if (f2a_fits(nvid, xoff, yoff, Hd, FWMAXQ)) return FX_X2Y_CORE_F2A_WIDE;
  return FX_X2Y_CORE_NONE;
}

long long x2y_f2a_chunks(int nvid, const int* xoff) {
  long long nch = 0;
  for (int v = 0; v < nvid; ++v) nch += (xoff[v + 1] - xoff[v] + FC - 1) / FC;
  return nch;
}

long long x2y_f2a_ws_floats(int nvid, const int* xoff, const int* yoff, int Hd) {
  return x2y_f2a_chunks(nvid, xoff) * f2a_qrows(nvid, yoff) * ((long long)Hd + 2);
}

int launch_x2y_f2a_fwd(const float* yq, const float* xk, const float* xv, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* logit, float* attn,
                       float* feat, float* ws, hipStream_t s) {
  FX_REQUIRE(f2a_fits(nvid, xoff, yoff, Hd, FWMAXQ), "x2y f2a core: <= 320 queries per video, Hd % 256 == 0");
  F2aArgs a{};
  a.yq = yq;
  a.xk = xk;
  a.xv = xv;
  a.logit = logit;
  a.attn = attn;
  a.feat = feat;
  a.scale = scale;
  const int nch = f2a_prepare(a, nvid, yoff, xoff, aoff, Hd, ws), maxq = x2y_max_rows(nvid, yoff);
  if (nch == 0 || maxq == 0) return FX_OK;
  if (maxq <= FMAXQ) {
    fx_launch(x2y_f2a_chunk_kernel<false>, dim3(nch), dim3(XT), 0, s, a);
    fx_launch(x2y_f2a_merge_kernel<false>, dim3(maxq, nvid), dim3(XT), 0, s, a);
  } else {
    fx_launch(x2y_f2a_chunk_kernel<true>, dim3(nch, a.qrows / FMAXQ), dim3(XT), 0, s, a);
    fx_launch(x2y_f2a_merge_kernel<true>, dim3(maxq, nvid), dim3(XT), 0, s, a);
  }
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_x2y_f2a_bwd(const float* dfeat, long long ldf, const float* xv, const float* xk, const float* yq,
                       const float* attn, const float* dattn, const float* dlogit_in, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* dlogit, float* dxv, float* dxk,
                       float* dyq, float* ws, unsigned* status, hipStream_t s) {
  FX_REQUIRE(f2a_fits(nvid, xoff, yoff, Hd, FWMAXQ), "x2y f2a core: <= 320 queries per video, Hd % 256 == 0");
  FX_REQUIRE(ldf % 4 == 0 && (reinterpret_cast<uintptr_t>(dfeat) & 15) == 0, "x2y f2a bwd: dfeat rows must be 16-B aligned");
  F2aBwdArgs a{};
  a.dfeat = dfeat;
  a.ldf = ldf;
  a.attn = attn;
  a.dattn = dattn;
  a.dl_in = dlogit_in;
  a.xv = xv;
  a.xk = xk;
  a.yq = yq;
  a.dL = dlogit;
  a.dxv = dxv;
  a.dxk = dxk;
  a.dyq = dyq;
  a.scale = scale;
  a.status = status;
  a.spin_max = x2y_spin_max();
  const int nch = f2a_prepare(a, nvid, yoff, xoff, aoff, Hd, ws), maxq = x2y_max_rows(nvid, yoff);
  if (nch == 0 || maxq == 0) return FX_OK;
  if (maxq > FMAXQ)
    f2a_bwd_launches<true>(a, nch, maxq, s);
  else
    f2a_bwd_launches<false>(a, nch, maxq, s);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx
