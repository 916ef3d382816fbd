// Verb / noun class heads of the EPIC-Kitchens FACT (fact_clip/models/blocks_SepVerbNoun.py):
//   process_feature with two softmax groups          (blocks_SepVerbNoun.py:227-232, basic.py:56-65)
//   verb/noun -> action log-probabilities + backward (blocks_SepVerbNoun.py:189-224)
//   TDU segmentation from the factorised probabilities (blocks_SepVerbNoun.py:285-296)
//
// Layout: every kernel works row by row and stages the row's n1 + n2 head values in LDS, because
// the action columns gather from them at random (EPIC: 98 + 301 heads, ~4k actions per row).
//   pf2 / argmax : one wave per row, 4 rows per workgroup, one LDS slice per wave
//   logp fwd/bwd : one 256-thread workgroup per row (the backward also stages the row's A (+1)
//                  upstream gradients, which the bins gather)
// Determinism: no float atomics.  Reductions are wave shuffles in a fixed tree plus a fixed-order
// combine of the 4 wave partials; the backward's scatter is a gather through inverse (CSR) lists,
// one thread per bin summing its actions in ascending order -- bitwise repeatable run to run.
#include "fx_common.h"
#include "ops.h"

namespace fx {
namespace {

constexpr int VN_MAXH = 2048;    // n1 + n2 head columns staged per row
constexpr int VN_MAXA = 12287;   // actions per mapping (+ the null column: 48 KiB of gradients in LDS)
constexpr int VN_THREADS = 256;

__device__ inline float vn_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline float vn_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------- process_feature, two groups
// softmax of sh[0, n) in place (one wave; the caller has made sh visible to the wave)
__device__ inline void vn_wave_softmax(float* sh, int n, int lane) {
  float m = -INFINITY;
  for (int c = lane; c < n; c += 64) m = fmaxf(m, sh[c]);
  m = vn_wave_max(m);
  float s = 0.f;
  for (int c = lane; c < n; c += 64) s += __expf(sh[c] - m);
  const float inv = 1.f / vn_wave_sum(s);
  for (int c = lane; c < n; c += 64) sh[c] = __expf(sh[c] - m) * inv;
}

__global__ __launch_bounds__(256) void pf2_fwd_kernel(const float* x, long long ldx, int rows, int cols, int n1,
                                                      int n2, float* out, long long ldo, float* clogit,
                                                      long long ldc) {
  __shared__ float head[4][VN_MAXH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wv;
  const bool on = row < rows;
  const int n = n1 + n2, f = cols - n;
  float* sh = head[wv];
  if (on) {
    const float* xr = x + (long long)row * ldx;
    float* orow = out + (long long)row * ldo;
    for (int c = lane; c < f; c += 64) orow[c] = xr[c];
    for (int c = lane; c < n; c += 64) {
      const float v = xr[f + c];
      sh[c] = v;
      if (clogit) clogit[(long long)row * ldc + c] = v;
    }
  }
  __syncthreads();
  if (on) vn_wave_softmax(sh, n1, lane);
  if (on) vn_wave_softmax(sh + n1, n2, lane);
  __syncthreads();
  if (on) {
    float* orow = out + (long long)row * ldo + f;
    for (int c = lane; c < n; c += 64) orow[c] = sh[c];
  }
}

__global__ __launch_bounds__(256) void pf2_bwd_kernel(const float* out, long long ldo, const float* dout,
                                                      long long lddo, const float* dcl, long long lddc, int rows,
                                                      int cols, int n1, int n2, float* dx, long long lddx) {
  __shared__ float head[4][VN_MAXH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wv;
  const bool on = row < rows;
  const int n = n1 + n2, f = cols - n;
  float* sh = head[wv];
  const float* orow = out + (long long)row * ldo;
  const float* drow = dout + (long long)row * lddo;
  float* xrow = dx + (long long)row * lddx;
  if (on) {
    for (int c = lane; c < f; c += 64) xrow[c] = drow[c];
    for (int c = lane; c < n; c += 64) sh[c] = orow[f + c];   // the row's probabilities
  }
  __syncthreads();
  if (on) {
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < n1; c += 64) s1 += sh[c] * drow[f + c];
    for (int c = n1 + lane; c < n; c += 64) s2 += sh[c] * drow[f + c];
    s1 = vn_wave_sum(s1);
    s2 = vn_wave_sum(s2);
    for (int c = lane; c < n; c += 64) {
      float v = sh[c] * (drow[f + c] - (c < n1 ? s1 : s2));
      if (dcl) v += dcl[(long long)row * lddc + c];
      xrow[f + c] = v;
    }
  }
}

// ---------------------------------------------------------------- verb/noun -> action log-probabilities
// block-wide max / sum of one value per thread: wave tree, then the 4 partials in fixed order
__device__ inline float vn_block_max(float v, float* part) {
  v = vn_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}
__device__ inline float vn_block_sum(float v, float* part) {
  v = vn_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// log-sum-exp of sh[0, n) over the workgroup
__device__ inline float vn_block_lse(const float* sh, int n, float* part) {
  float m = -INFINITY;
  for (int c = threadIdx.x; c < n; c += VN_THREADS) m = fmaxf(m, sh[c]);
  m = vn_block_max(m, part);
  float s = 0.f;
  for (int c = threadIdx.x; c < n; c += VN_THREADS) s += expf(sh[c] - m);
  s = vn_block_sum(s, part);
  return m + logf(s);
}

__global__ __launch_bounds__(VN_THREADS) void vn_logp_fwd_kernel(const float* clogit, long long ldc, int n1, int n2,
                                                                 const int32_t* vids, const int32_t* nids, int A,
                                                                 int null, float* logp, long long ldl, float* lse) {
  __shared__ float sh[VN_MAXH];
  __shared__ float part[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int n = n1 + n2;
  const float* cr = clogit + (long long)row * ldc;
  for (int c = tid; c < n; c += VN_THREADS) sh[c] = cr[c];
  __syncthreads();
  const float lv = vn_block_lse(sh, n1, part);
  const float ln = vn_block_lse(sh + n1, n2, part);
  __syncthreads();
  for (int c = tid; c < n; c += VN_THREADS) sh[c] -= (c < n1 ? lv : ln);   // log-softmax of both groups
  __syncthreads();
  float* lr = logp + (long long)row * ldl;
  for (int a = tid; a < A; a += VN_THREADS) {
    const int v = min(max(vids[a], 0), n1 - 1), k = min(max(nids[a], 0), n2 - 1);
    lr[a] = sh[v] + sh[n1 + k];
  }
  if (tid == 0) {
    if (null) lr[A] = sh[n1 - 1] + sh[n - 1];
    lse[2 * (long long)row] = lv;
    lse[2 * (long long)row + 1] = ln;
  }
}

// dclogit[j] = sum_{a in bin j} g[a] (ascending a; the null column last, into the last bin of each
// group) - softmax[j] * sum_a g[a]
__global__ __launch_bounds__(VN_THREADS) void vn_logp_bwd_kernel(const float* clogit, long long ldc, const float* lse,
                                                                 const float* g, long long ldg, int n1, int n2, int A,
                                                                 int null, const int32_t* voff, const int32_t* vlist,
                                                                 const int32_t* noff, const int32_t* nlist,
                                                                 float* dcl, long long lddc) {
  extern __shared__ float gs[];   // A + null upstream gradients of the row
  __shared__ float part[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int n = n1 + n2, Ao = A + (null ? 1 : 0);
  const float* gr = g + (long long)row * ldg;
  float tot = 0.f;
  for (int a = tid; a < Ao; a += VN_THREADS) {
    const float v = gr[a];
    gs[a] = v;
    tot += v;
  }
  tot = vn_block_sum(tot, part);   // (its barriers also publish gs)
  const float lv = lse[2 * (long long)row], ln = lse[2 * (long long)row + 1];
  const float* cr = clogit + (long long)row * ldc;
  float* dr = dcl + (long long)row * lddc;
  for (int j = tid; j < n; j += VN_THREADS) {
    const bool verb = j < n1;
    const int b = verb ? j : j - n1;
    const int32_t* off = verb ? voff : noff;
    const int32_t* lst = verb ? vlist : nlist;
    float s = 0.f;
    const int e = min(off[b + 1], A);
    for (int i = max(off[b], 0); i < e; ++i) s += gs[min(max(lst[i], 0), A - 1)];
    if (null && b == (verb ? n1 : n2) - 1) s += gs[A];
    dr[j] = s - expf(cr[j] - (verb ? lv : ln)) * tot;
  }
}

// ---------------------------------------------------------------- TDU argmax over factorised probabilities
// pred[t] = argmax_a x[t, col0 + vids[a]] * x[t, col0 + n1 + nids[a]]  (fp32 product, first maximum)
__global__ __launch_bounds__(256) void argmax_vn_kernel(const float* x, long long ldx, int col0, int n1, int n2,
                                                        const int32_t* vids, const int32_t* nids, int A, int T,
                                                        int32_t* pred) {
  __shared__ float head[4][VN_MAXH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wv;
  const bool on = t < T;
  const int n = n1 + n2;
  float* sh = head[wv];
  if (on) {
    const float* xr = x + (long long)t * ldx + col0;
    for (int c = lane; c < n; c += 64) sh[c] = xr[c];
  }
  __syncthreads();
  if (!on) return;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int a = lane; a < A; a += 64) {
    const int v = min(max(vids[a], 0), n1 - 1), k = min(max(nids[a], 0), n2 - 1);
    const float p = __fmul_rn(sh[v], sh[n1 + k]);
    if (p > best) {  // lanes visit increasing a: keeps the first max per lane
      best = p;
      bi = a;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) pred[t] = (bi == 0x7fffffff) ? 0 : bi;
}

}  // namespace

static int vn_check_heads(int n1, int n2) {
  FX_REQUIRE(n1 > 0 && n2 > 0 && n1 + n2 <= VN_MAXH, "verb/noun heads: need n1, n2 > 0 and n1 + n2 <= 2048");
  return FX_OK;
}

int launch_pf2_fwd(const float* x, long long ldx, int rows, int cols, int n1, int n2, float* out, long long ldo,
                   float* clogit, long long ldc, hipStream_t s) {
  FX_TRY(vn_check_heads(n1, n2));
  FX_REQUIRE(n1 + n2 <= cols && rows >= 0, "process_feature2: need n1 + n2 <= cols");
  if (rows == 0) return FX_OK;
  fx_launch(pf2_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, ldx, rows, cols, n1, n2, out, ldo, clogit, ldc);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_pf2_bwd(const float* out, long long ldo, const float* dout, long long lddo, const float* dcl,
                   long long lddc, int rows, int cols, int n1, int n2, float* dx, long long lddx, hipStream_t s) {
  FX_TRY(vn_check_heads(n1, n2));
  FX_REQUIRE(n1 + n2 <= cols && rows >= 0, "process_feature2: need n1 + n2 <= cols");
  if (rows == 0) return FX_OK;
  fx_launch(pf2_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, out, ldo, dout, lddo, dcl, lddc, rows, cols, n1,
            n2, dx, lddx);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_vn_logp_fwd(const float* clogit, long long ldc, int rows, int n1, int n2, const int32_t* vids,
                       const int32_t* nids, int A, int null, float* logp, long long ldl, float* lse,
                       hipStream_t s) {
  FX_TRY(vn_check_heads(n1, n2));
  FX_REQUIRE(A > 0 && A <= VN_MAXA && rows >= 0, "vn_logp: need 0 < A <= 12287 actions");
  FX_REQUIRE(ldc >= n1 + n2 && ldl >= A + (null ? 1 : 0), "vn_logp: leading dimension shorter than the row");
  if (rows == 0) return FX_OK;
  fx_launch(vn_logp_fwd_kernel, dim3(rows), dim3(VN_THREADS), 0, s, clogit, ldc, n1, n2, vids, nids, A, null, logp,
            ldl, lse);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_vn_logp_bwd(const float* clogit, long long ldc, const float* lse, const float* dlogp, long long ldg,
                       int rows, int n1, int n2, int A, int null, const int32_t* voff, const int32_t* vlist,
                       const int32_t* noff, const int32_t* nlist, float* dclogit, long long lddc, hipStream_t s) {
  FX_TRY(vn_check_heads(n1, n2));
  FX_REQUIRE(A > 0 && A <= VN_MAXA && rows >= 0, "vn_logp: need 0 < A <= 12287 actions");
  FX_REQUIRE(ldc >= n1 + n2 && lddc >= n1 + n2 && ldg >= A + (null ? 1 : 0),
             "vn_logp: leading dimension shorter than the row");
  if (rows == 0) return FX_OK;
  const std::uint32_t shm = (std::uint32_t)((A + 1) * sizeof(float));
  fx_launch(vn_logp_bwd_kernel, dim3(rows), dim3(VN_THREADS), shm, s, clogit, ldc, lse, dlogp, ldg, n1, n2, A, null,
            voff, vlist, noff, nlist, dclogit, lddc);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_segments_vn(const float* x, long long ldx, int col0, int n1, int n2, const int32_t* vids,
                       const int32_t* nids, int A, int T, int nvid, const int* row_off, int32_t* pred,
                       int32_t* seg_id, int32_t* seg_start, int32_t* seg_end, int32_t* num_seg, hipStream_t s) {
  FX_TRY(vn_check_heads(n1, n2));
  FX_REQUIRE(A > 0 && col0 >= 0, "segments (verb/noun): need A > 0 actions and col0 >= 0");
  int rows = 0;
  FX_TRY(segments_check_rows(T, nvid, row_off, &rows));
  fx_launch(argmax_vn_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, ldx, col0, n1, n2, vids, nids, A, rows, pred);
  return launch_boundary_scan(pred, T, nvid, row_off, seg_id, seg_start, seg_end, num_seg, s);
}

}  // namespace fx
