// Fused multi-head attention for token-sized problems (Lq, Lk, head_dim <= 64): the
// nn.MultiheadAttention core of SALayer / SCALayer's self-attention over the Q = Nact action
// tokens (basic.py:442, 500).  One workgroup per head holds Q_h, K_h, V_h, P_h in LDS, so the
// whole forward (S = scale * Q K^T, row softmax, O = P V) or backward (dP = dO V^T,
// dS = P * (dP - rowsum(P * dP)), dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO) is ONE launch
// instead of three batched GEMMs + a softmax (+ split-K reduces).  At 32 x 32 x 32 per head the
// work is ~100 k FMAs per workgroup: latency-bound, so plain fp32 FMAs from LDS (exact f32
// products like the reference CPU path), no MFMA tiling.
#include <algorithm>
#include <cmath>

#include "fx_common.h"
#include "ops.h"
#include "wave_dev.h"

namespace fx {
namespace {

constexpr int SM = 64;        // max Lq, Lk, head_dim
constexpr int SP = SM + 1;    // padded LDS row stride (no bank conflicts on column walks)
// 1024 threads: each output element is one thread's serial FMA chain (fixed order, so the result does
// not depend on NT); at Breakfast's 60 tokens x head dim 64 a 256-thread block left each thread ~15
// elements of 64-deep chains (bwd 72 us per launch over only heads x videos = 32 workgroups)
constexpr int NT = 1024;

constexpr int MAXV = 32;      // videos per launch (the per-video row offsets live in the kernel arguments)

// rows of video v: q / o rows [qo[v], qo[v+1]), k / v rows [ko[v], ko[v+1]) (the host fills v*Lq, v*Lk for
// an even split); Lq, Lk are the longest video's counts (the saved probabilities' per-video block)
struct SmallOff {
  int qo[MAXV + 1];
  int ko[MAXV + 1];
};

// keep-scale of probability (head h, global query row qg, global key row kg of ktot): 1/(1-p) or 0 -- the
// attention-over-T kernels' mask (attn_t_dev.h drop_keep)
__device__ __forceinline__ float keep_scale(unsigned long long seed, unsigned thr, float p, int nh, int h,
                                            unsigned long long qg, unsigned long long kg, unsigned long long ktot) {
  const unsigned long long idx = (qg * nh + h) * ktot + kg;
  return fx_drop_bits(seed, idx) >= thr ? 1.f / (1.f - p) : 0.f;
}

__device__ __forceinline__ void load_tile(float (*dst)[SP], const float* src, long long ld, int rows, int cols) {
  for (int e = threadIdx.x; e < rows * cols; e += NT) {
    const int r = e / cols, c = e - r * cols;
    dst[r][c] = src[(long long)r * ld + c];
  }
}

__global__ __launch_bounds__(NT) void mha_small_fwd_kernel(const float* q, long long ldq, const float* k,
                                                           long long ldk, const float* v, long long ldv, int Lq,
                                                           int Lk, int hd, float scale, float* probs, float* o,
                                                           long long ldo, float drop_p, unsigned thr,
                                                           unsigned long long seed, SmallOff off) {
  __shared__ float Qs[SM][SP], Ks[SM][SP], Vs[SM][SP], Ps[SM][SP];
  const int h = blockIdx.x, vid = blockIdx.y;   // head, video (rows qo[vid].. of q/o, ko[vid].. of k/v)
  const int q0 = off.qo[vid], k0 = off.ko[vid], ktot = off.ko[gridDim.y];
  probs += (long long)vid * gridDim.x * Lq * Lk;   // per-video block sized by the longest video, dense inside
  Lq = off.qo[vid + 1] - q0;
  Lk = off.ko[vid + 1] - k0;
  q += (long long)q0 * ldq;
  k += (long long)k0 * ldk;
  v += (long long)k0 * ldv;
  o += (long long)q0 * ldo;
  load_tile(Qs, q + h * hd, ldq, Lq, hd);
  load_tile(Ks, k + h * hd, ldk, Lk, hd);
  load_tile(Vs, v + h * hd, ldv, Lk, hd);
  __syncthreads();
  for (int e = threadIdx.x; e < Lq * Lk; e += NT) {
    const int i = e / Lk, j = e - i * Lk;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc += Qs[i][d] * Ks[j][d];
    Ps[i][j] = acc * scale;
  }
  __syncthreads();
  // row softmax: one wave per row
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = w; i < Lq; i += NT / 64) {
    const float x = lane < Lk ? Ps[i][lane] : -INFINITY;
    const float m = wmax(x);
    const float ex = lane < Lk ? __expf(x - m) : 0.f;
    const float p = ex / wsum(ex);
    if (lane < Lk) {
      probs[((long long)h * Lq + i) * Lk + lane] = p;   // saved before dropout (backward recomputes the mask)
      Ps[i][lane] = drop_p > 0.f ? p * keep_scale(seed, thr, drop_p, gridDim.x, h, q0 + i, k0 + lane, ktot) : p;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < Lq * hd; e += NT) {
    const int i = e / hd, d = e - i * hd;
    float acc = 0.f;
    for (int j = 0; j < Lk; ++j) acc += Ps[i][j] * Vs[j][d];
    o[(long long)i * ldo + h * hd + d] = acc;
  }
}

__global__ __launch_bounds__(NT) void mha_small_bwd_kernel(const float* q, long long ldq, const float* k,
                                                           long long ldk, const float* v, long long ldv,
                                                           const float* probs, const float* dout, long long lddo,
                                                           int Lq, int Lk, int hd, float scale, float* dq,
                                                           long long lddq, float* dk, long long lddk, float* dv,
                                                           long long lddv, float drop_p, unsigned thr,
                                                           unsigned long long seed, SmallOff off) {
  __shared__ float Qs[SM][SP], Ks[SM][SP], Vs[SM][SP], Ps[SM][SP], Ds[SM][SP], Gs[SM][SP];
  __shared__ float Ms[SM][SP];   // dropout keep-scales (training only)
  const int h = blockIdx.x, vid = blockIdx.y;
  const int q0 = off.qo[vid], k0 = off.ko[vid], ktot = off.ko[gridDim.y];
  probs += (long long)vid * gridDim.x * Lq * Lk;
  Lq = off.qo[vid + 1] - q0;
  Lk = off.ko[vid + 1] - k0;
  q += (long long)q0 * ldq;
  k += (long long)k0 * ldk;
  v += (long long)k0 * ldv;
  dout += (long long)q0 * lddo;
  if (dq) dq += (long long)q0 * lddq;
  if (dk) dk += (long long)k0 * lddk;
  if (dv) dv += (long long)k0 * lddv;
  load_tile(Qs, q + h * hd, ldq, Lq, hd);
  load_tile(Ks, k + h * hd, ldk, Lk, hd);
  load_tile(Vs, v + h * hd, ldv, Lk, hd);
  load_tile(Ps, probs + (long long)h * Lq * Lk, Lk, Lq, Lk);
  load_tile(Ds, dout + h * hd, lddo, Lq, hd);   // dO_h
  const bool drop = drop_p > 0.f;
  if (drop)
    for (int e = threadIdx.x; e < Lq * Lk; e += NT) {
      const int i = e / Lk, j = e - i * Lk;
      Ms[i][j] = keep_scale(seed, thr, drop_p, gridDim.x, h, q0 + i, k0 + j, ktot);
    }
  __syncthreads();
  // dP = dO V^T  -> Gs
  for (int e = threadIdx.x; e < Lq * Lk; e += NT) {
    const int i = e / Lk, j = e - i * Lk;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc += Ds[i][d] * Vs[j][d];
    Gs[i][j] = drop ? acc * Ms[i][j] : acc;   // gradient of the un-dropped P
  }
  __syncthreads();
  // dV = P_d^T dO with P_d the dropped probabilities (uses Ps, Ds before they are overwritten)
  if (dv)
    for (int e = threadIdx.x; e < Lk * hd; e += NT) {
      const int j = e / hd, d = e - j * hd;
      float acc = 0.f;
      if (drop)
        for (int i = 0; i < Lq; ++i) acc += Ps[i][j] * Ms[i][j] * Ds[i][d];
      else
        for (int i = 0; i < Lq; ++i) acc += Ps[i][j] * Ds[i][d];
      dv[(long long)j * lddv + h * hd + d] = acc;
    }
  // dS = P * (dP - rowsum(P dP)), one wave per row, in place in Gs
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = w; i < Lq; i += NT / 64) {
    const float p = lane < Lk ? Ps[i][lane] : 0.f;
    const float g = lane < Lk ? Gs[i][lane] : 0.f;
    const float r = wsum(p * g);
    if (lane < Lk) Gs[i][lane] = p * (g - r);
  }
  __syncthreads();
  if (dq)
    for (int e = threadIdx.x; e < Lq * hd; e += NT) {
      const int i = e / hd, d = e - i * hd;
      float acc = 0.f;
      for (int j = 0; j < Lk; ++j) acc += Gs[i][j] * Ks[j][d];
      dq[(long long)i * lddq + h * hd + d] = acc * scale;
    }
  if (dk)
    for (int e = threadIdx.x; e < Lk * hd; e += NT) {
      const int j = e / hd, d = e - j * hd;
      float acc = 0.f;
      for (int i = 0; i < Lq; ++i) acc += Gs[i][j] * Qs[i][d];
      dk[(long long)j * lddk + h * hd + d] = acc * scale;
    }
}

// the offsets table: `off` (host, nvid + 1, self-attention: q and k/v rows alike, Lq = Lk the longest
// video) or the even split
int small_off(SmallOff& t, const int* off, int nvid, int Lq, int Lk) {
  FX_REQUIRE(nvid >= 1 && nvid <= MAXV, "mha_small: 1..32 videos");
  int mx = 0;
  for (int v = 0; v <= nvid; ++v) {
    t.qo[v] = off ? off[v] : v * Lq;
    t.ko[v] = off ? off[v] : v * Lk;
    if (v > 0) {
      FX_REQUIRE(t.qo[v] > t.qo[v - 1], "mha_small: row offsets must increase");
      mx = std::max(mx, t.qo[v] - t.qo[v - 1]);
    }
  }
  FX_REQUIRE(!off || (off[0] == 0 && Lq == Lk && mx <= Lq), "mha_small: row offsets start at 0, within the longest video");
  return FX_OK;
}

}  // namespace

int launch_mha_small_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                         int Lq, int Lk, int hd, int nhead, float scale, float* probs, float* o, long long ldo,
                         hipStream_t s, int nvid, float drop_p, unsigned long long seed, const int* off) {
  FX_REQUIRE(Lq > 0 && Lk > 0 && hd > 0 && Lq <= SM && Lk <= SM && hd <= SM && nhead > 0,
             "mha_small: Lq, Lk, head_dim must be in [1, 64]");
  SmallOff t{};
  FX_TRY(small_off(t, off, nvid, Lq, Lk));
  FX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "mha_small: dropout p in [0, 1)");
  const unsigned thr = drop_p > 0.f ? std::max(fx_drop_thresh(drop_p), 1u) : 0u;
  fx_launch(mha_small_fwd_kernel, dim3(nhead, nvid), dim3(NT), 0, s, q, ldq, k, ldk, v, ldv, Lq, Lk, hd, scale,
                     probs, o, ldo, drop_p, thr, seed, t);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_mha_small_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                         const float* probs, const float* dout, long long lddo, int Lq, int Lk, int hd, int nhead,
                         float scale, float* dq, long long lddq, float* dk, long long lddk, float* dv, long long lddv,
                         hipStream_t s, int nvid, float drop_p, unsigned long long seed, const int* off) {
  FX_REQUIRE(Lq > 0 && Lk > 0 && hd > 0 && Lq <= SM && Lk <= SM && hd <= SM && nhead > 0,
             "mha_small: Lq, Lk, head_dim must be in [1, 64]");
  SmallOff t{};
  FX_TRY(small_off(t, off, nvid, Lq, Lk));
  FX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "mha_small: dropout p in [0, 1)");
  const unsigned thr = drop_p > 0.f ? std::max(fx_drop_thresh(drop_p), 1u) : 0u;
  fx_launch(mha_small_bwd_kernel, dim3(nhead, nvid), dim3(NT), 0, s, q, ldq, k, ldk, v, ldv, probs, dout, lddo,
                     Lq, Lk, hd, scale, dq, lddq, dk, lddk, dv, lddv, drop_p, thr, seed, t);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx
