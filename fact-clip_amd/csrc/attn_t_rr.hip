// Attention of a few queries over T frames (see attn_t_lds.hip for the algorithm): the register-resident
// kernel family.  For head dim 32, <= 32 queries per video and 16-B aligned rows (the benchmark's SCA
// decoder: 8 heads of 32, 32 tokens; tattn_plan, attention.cpp, makes the choice) every operand goes
// straight from memory into MFMA registers, no LDS staging:
//   * S^T (keys x queries) = K q^T: lane (li, lh) feeds K[key li][16 lh .. 16 lh + 15] and
//     q[query li][16 lh ..] as A / B (4 float4 each; the d order inside the sum is free as long as A and
//     B agree);
//   * the S^T accumulators hold, per lane, 16 keys of ONE query (keys acc_row(r)): the softmax statistics
//     are in-register reductions plus one exchange with the other lane half;
//   * O^T (d x queries) = V^T P^T takes the probabilities straight from those accumulators as the B
//     operand, the key of MFMA step j being acc_row(j) -- V[key acc_row(j)][d li] as the A operand (32
//     lanes read one 128-B row slice);
//   * each wave owns 32 KT keys of the chunk; the 4 waves' (m, l, O) are combined through LDS once.
// Backward: S^T and dP^T = V dO^T the same way, dq = dS K with dS^T from the accumulators as the A
// operand; dV = P_d^T dO and dK = scale dS^T q need the probabilities with the key as the ROW index, so
// P_d^T and dS^T go through a wave-private LDS tile (no workgroup barrier).
// The chunk partials of a (video, head) are merged inside the launch by its last workgroup to finish
// (fold_merge: faster here than the second launch) when the plan says so and the stream has
// arrival counters (a.cnt); otherwise they are left in the workspace for tattn_merge_kernel.
#include <cmath>

#include "attn_t_dev.h"

namespace fx {
namespace {
using namespace attn_t_dev;

__device__ __forceinline__ float4 ld4g(const float* p) { return *reinterpret_cast<const float4*>(p); }
// Diagnostic builds only (-DTATTN_STAMPS, tools/tattn_stamps.py): s_memrealtime stamps of thread 0 of every
// workgroup of the last tattn_fwd32_kernel launch (fx_debug_tattn_stamps); never in the shipped library
#ifdef TATTN_STAMPS
__device__ unsigned long long g_ta_st[1024 * 8];
#define TA_ST(k)                                                                                        \
  do {                                                                                                  \
    const int b_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                      \
    if (threadIdx.x == 0 && b_ < 1024) g_ta_st[b_ * 8 + (k)] = __builtin_amdgcn_s_memrealtime();        \
  } while (0)
#else
#define TA_ST(k) \
  do {           \
  } while (0)
#endif

// The chunk partials of (video, head) merged by the LAST workgroup to finish one (the microarch guide's
// write-through hand-off, valid form 1): every workgroup stored its 32 x 32 partial (and forward: row
// max / sum) with sc1 stores and waited for their acknowledgement before its arrival on the counter; the
// last arriver re-arms the counter and reads the partials with sc1 loads, in chunk order (deterministic,
// the same order as tattn_merge_kernel).  Forward (stats): o = sum_s e^(m_s - M) O_s / L, lse = M + log L;
// backward: dq = mul sum_s dq_s.  Returns after the merge (or at once for the other workgroups).
__device__ __forceinline__ void fold_merge(const TAttnArgs& a, int vid, int h, int ns, bool stats, float mul,
                                           long long qrow, float (*wm)[32], float (*wl)[32]) {
  __shared__ int last;
  const int tid = threadIdx.x;
  const int Qn = live_queries(a, vid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's partial stores acknowledged
  __syncthreads();
  if (stats) TA_ST(4);
  if (tid == 0) {
    unsigned* c = a.cnt + (long long)vid * a.nh + h;
    const unsigned prev = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == (unsigned)ns - 1;
    if (last) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (stats) TA_ST(5);
  if (!last) return;
  const TAttnWs W(gridDim.z, a.nh, a.nsplit, 32, 32);
  const long long pbase = TAttnWs::pid(vid, a.nh, h, a.nsplit, 0);
  const float* part = a.ws;
  const float* pm = a.ws + W.m();
  const float* pl = a.ws + W.l();
  // every load of the merge at once: this thread's (query, 4 consecutive d) slice of every partial as one
  // 16-B load each (query tid / 8, d 4 (tid % 8) ..), and (forward) the row statistics of (partial, query)
  // pairs tid, tid + 256
  const int mq = tid >> 3, md = (tid & 7) * 4;
  float4 x[FOLD_MAX];
#pragma unroll
  for (int sp = 0; sp < FOLD_MAX; ++sp) x[sp] = ldc4(part, W.at(pbase + min(sp, ns - 1), mq, md));
  if (stats) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + i * AT, sp = e >> 5, q = e & 31;
      const float m = ldc1(pm, (pbase + min(sp, ns - 1)) * 32 + q), l = ldc1(pl, (pbase + min(sp, ns - 1)) * 32 + q);
      if (sp < ns) {
        wm[sp][q] = m;
        wl[sp][q] = l;
      }
    }
    __syncthreads();
    if (tid < 32) {
      float M = -INFINITY;
      for (int sp = 0; sp < ns; ++sp) M = fmaxf(M, wm[sp][tid]);
      float L = 0.f;
      for (int sp = 0; sp < ns; ++sp) L += __expf(wm[sp][tid] - M) * wl[sp][tid];
      const float inv = 1.f / L;
      for (int sp = 0; sp < ns; ++sp) wm[sp][tid] = __expf(wm[sp][tid] - M) * inv;
      if (tid < Qn) a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + tid] = M + __logf(L);
    }
    __syncthreads();
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int sp = 0; sp < FOLD_MAX; ++sp)
    if (sp < ns) {
      const float wgt = stats ? wm[sp][mq] : 1.f;
      acc.x += wgt * x[sp].x;
      acc.y += wgt * x[sp].y;
      acc.z += wgt * x[sp].z;
      acc.w += wgt * x[sp].w;
    }
  if (mq < Qn) {
    float* o = a.out + (qrow + mq) * a.ld_out + h * 32 + md;
    o[0] = acc.x * mul;
    o[1] = acc.y * mul;
    o[2] = acc.z * mul;
    o[3] = acc.w * mul;
  }
  if (stats) TA_ST(6);
}

// Where one thread's 16 B (query q, d0 .. d0 + 3) of its workgroup's 32 x 32 result go, and with STATS
// (forward) the query's row max / sum from the thread with d0 == 0:
//   * false, nothing stored: a one-chunk video (ns == 1), whose rows the caller writes directly -- except
//     when a merge launch follows (no a.cnt, more than one chunk in the launch): that launch merges every
//     video, so every video leaves partials;
//   * partial (vid, h, c) of the workspace with sc1 write-through stores when the merge runs in this launch
//     (a.cnt), with plain stores for the merge launch.
template <bool STATS>
__device__ __forceinline__ bool store_partial(const TAttnArgs& a, int vid, int h, int c, int ns, int q, int d0,
                                              float4 v, float M, float L) {
  const TAttnWs W(gridDim.z, a.nh, a.nsplit, 32, 32);
  const long long pid = TAttnWs::pid(vid, a.nh, h, a.nsplit, c);
  float* pm = a.ws + W.m();
  float* pl = a.ws + W.l();
  const bool fold = a.cnt != nullptr;
  if (ns == 1 && (fold || a.nsplit == 1)) return false;
  if (fold) {
    stc4(a.ws, W.at(pid, q, d0), v);
    if (STATS && d0 == 0) {
      stc1(pm, pid * 32 + q, M);
      stc1(pl, pid * 32 + q, L);
    }
  } else {
    *reinterpret_cast<float4*>(a.ws + W.at(pid, q, d0)) = v;
    if (STATS && d0 == 0) {
      pm[pid * 32 + q] = M;
      pl[pid * 32 + q] = L;
    }
  }
  return true;
}

template <int KT>
__global__ __launch_bounds__(AT) void tattn_fwd32_kernel(TAttnArgs a) {
  __shared__ float xo[4][32][33];   // per-wave O^T partial [d][query]
  __shared__ float xm[4][32], xl[4][32];
  const int c = blockIdx.x, h = blockIdx.y, vid = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  TA_ST(0);
  const auto [Tv, t0, nk, Qn, qrow, krow] = tattn_chunk(a, c, vid);   // Qn >= 1: one query block (q0 = 0)
  if (nk <= 0) return;
  const int kw0 = w * 32 * KT;                    // this wave's first key of the chunk
  // every load first: q and K fragments, V columns
  float4 qf[4], kf[KT][4];
  float vf[KT][16];
  {
    const float* qp = a.q + (qrow + min(li, Qn - 1)) * a.ldq + h * 32 + 16 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) qf[q] = ld4g(qp + 4 * q);
    // (every K fragment before the first V column: loads complete in issue order, so S = q K^T then waits
    // for K alone and the V columns arrive behind its MFMAs)
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      const float* kp = a.k + (krow + min(kw0 + 32 * u + li, nk - 1)) * a.ldk + h * 32 + 16 * lh;
#pragma unroll
      for (int q = 0; q < 4; ++q) kf[u][q] = ld4g(kp + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        vf[u][j] = a.v[(krow + min(kw0 + 32 * u + acc_row(j, lane), nk - 1)) * a.ldv + h * 32 + li];
    }
  }
  f32x16 st[KT];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < KT; ++u) {
    zero16(st[u]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      st[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].x, qf[q].x, st[u], 0, 0, 0);
      st[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].y, qf[q].y, st[u], 0, 0, 0);
      st[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].z, qf[q].z, st[u], 0, 0, 0);
      st[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].w, qf[q].w, st[u], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kw0 + 32 * u + acc_row(r, lane);
      st[u][r] = key < nk ? st[u][r] * a.scale : -INFINITY;
      mx = fmaxf(mx, st[u][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  TA_ST(1);
  float l = 0.f;
  f32x16 ou[KT];   // one P V accumulator per key tile: independent MFMA chains, summed after
#pragma unroll
  for (int u = 0; u < KT; ++u) {
    zero16(ou[u]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = mx == -INFINITY ? 0.f : __expf(st[u][r] - mx);   // (a wave past the video's keys)
      l += p;                                                         // the normaliser sees every key
      float kp = 1.f;
      if (a.drop_p > 0.f && p != 0.f) kp = drop_keep(a, qrow + li, h, krow + kw0 + 32 * u + acc_row(r, lane));
      st[u][r] = p * kp;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) ou[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u][j], st[u][j], ou[u], 0, 0, 0);
  }
  f32x16 o = ou[0];
#pragma unroll
  for (int u = 1; u < KT; ++u) o += ou[u];
  l += __shfl_xor(l, 32, 64);
  if (lane < 32) {
    xm[w][li] = mx;
    xl[w][li] = l;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) xo[w][acc_row(r, lane)][li] = o[r];
  TA_ST(2);
  __syncthreads();
  // the 4 waves' partials, in wave order; thread -> (query q, d) pairs
  const int ns = (Tv + a.Tc - 1) / a.Tc;   // this video's chunks
  {   // thread -> (query tid / 8, 4 consecutive d): one 16-B partial store (the merge reads it back the same way)
    const int q = tid >> 3, d0 = (tid & 7) * 4;
    float M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, xm[ww][q]);
    float4 O = make_float4(0.f, 0.f, 0.f, 0.f);
    float L = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float f = xm[ww][q] == -INFINITY ? 0.f : __expf(xm[ww][q] - M);
      O.x += f * xo[ww][d0][q];
      O.y += f * xo[ww][d0 + 1][q];
      O.z += f * xo[ww][d0 + 2][q];
      O.w += f * xo[ww][d0 + 3][q];
      L += f * xl[ww][q];
    }
    if (!store_partial<true>(a, vid, h, c, ns, q, d0, O, M, L) && q < Qn) {
      float* op = a.out + (qrow + q) * a.ld_out + h * 32 + d0;
      op[0] = O.x / L;
      op[1] = O.y / L;
      op[2] = O.z / L;
      op[3] = O.w / L;
      if (d0 == 0) a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + q] = M + __logf(L);
    }
  }
  TA_ST(3);
  if (ns > 1 && a.cnt)   // (the wave partial images are free now: the merge's weights reuse them)
    fold_merge(a, vid, h, ns, true, 1.f, qrow, reinterpret_cast<float(*)[32]>(&xo[0][0][0]),
               reinterpret_cast<float(*)[32]>(&xo[2][0][0]));
}

template <int KT>
__global__ __launch_bounds__(AT) void tattn_bwd32_kernel(TAttnArgs a) {
  __shared__ float tp[4][32][33];    // wave-private: P_d^T of the current key tile [key][query]
  __shared__ float tds[4][32][33];   // dS^T [key][query]
  __shared__ float xq[4][32][33];    // per-wave dq partial [query][d]
  const int c = blockIdx.x, h = blockIdx.y, vid = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const auto [Tv, t0, nk, Qn, qrow, krow] = tattn_chunk(a, c, vid);   // Qn >= 1: one query block (q0 = 0)
  if (nk <= 0) return;
  const int kw0 = w * 32 * KT;                    // this wave's first key of the chunk
  // every load first.  Query-side fragments (query li, d 16 lh ..): q, dO, o; query-side columns (query
  // acc_row(j), d li): q, dO (the B operands of dK and dV); key side: K and V fragments (key li, d 16 lh ..)
  // and K columns (key acc_row(j), d li) for dq
  float4 qf[4], df[4], of[4], kf[KT][4], vf[KT][4];
  float qt[16], dt[16], kt[KT][16];
  const int qi = min(li, Qn - 1);
  {
    const float* qp = a.q + (qrow + qi) * a.ldq + h * 32 + 16 * lh;
    const float* dp = a.dout + (qrow + qi) * a.lddo + h * 32 + 16 * lh;
    const float* op = a.o + (qrow + qi) * a.ldo + h * 32 + 16 * lh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      qf[q] = ld4g(qp + 4 * q);
      df[q] = ld4g(dp + 4 * q);
      of[q] = ld4g(op + 4 * q);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long qr = qrow + min(acc_row(j, lane), Qn - 1);
      qt[j] = a.q[qr * a.ldq + h * 32 + li];
      dt[j] = a.dout[qr * a.lddo + h * 32 + li];
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      const long long kr = krow + min(kw0 + 32 * u + li, nk - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        kf[u][q] = ld4g(a.k + kr * a.ldk + h * 32 + 16 * lh + 4 * q);
        vf[u][q] = ld4g(a.v + kr * a.ldv + h * 32 + 16 * lh + 4 * q);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        kt[u][j] = a.k[(krow + min(kw0 + 32 * u + acc_row(j, lane), nk - 1)) * a.ldk + h * 32 + li];
    }
  }
  const float lse = li < Qn ? a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + li] : 0.f;
  // D = rowsum(dO o) of this lane's query
  float D = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) D += (df[q].x * of[q].x + df[q].y * of[q].y) + (df[q].z * of[q].z + df[q].w * of[q].w);
  D += __shfl_xor(D, 32, 64);
  f32x16 dqu[KT];   // one dq accumulator per key tile (independent chains), summed after
#pragma unroll
  for (int u = 0; u < KT; ++u) {
    zero16(dqu[u]);
    f32x16 s, dp;
    zero16(s);
    zero16(dp);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].x, qf[q].x, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u][q].x, df[q].x, dp, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].y, qf[q].y, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u][q].y, df[q].y, dp, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].z, qf[q].z, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u][q].z, df[q].z, dp, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][q].w, qf[q].w, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[u][q].w, df[q].w, dp, 0, 0, 0);
    }
    // P^T, P_d^T, dS^T = P (dP keep - D) (dropout: P_d = P keep multiplied V, dP = (dO V^T) keep)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = acc_row(r, lane), key = kw0 + 32 * u + kl;
      const float p = (key < nk && li < Qn) ? __expf(s[r] * a.scale - lse) : 0.f;
      const float kp = (a.drop_p > 0.f && p != 0.f) ? drop_keep(a, qrow + li, h, krow + key) : 1.f;
      const float ds = p * (dp[r] * kp - D);
      tp[w][kl][li] = p * kp;
      tds[w][kl][li] = ds;
      s[r] = ds;
    }
    // dq += dS K: A = dS (query li, key acc_row(j)) from the accumulators, B = K (key acc_row(j), d li)
#pragma unroll
    for (int j = 0; j < 16; ++j) dqu[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[j], kt[u][j], dqu[u], 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's tile writes are visible to its lanes
    // dV = P_d^T dO and dK = dS^T q over the queries: A = the LDS tile (key li, query acc_row(j))
    f32x16 dv, dk;
    zero16(dv);
    zero16(dk);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int qj = acc_row(j, lane);
      dv = __builtin_amdgcn_mfma_f32_32x32x2f32(tp[w][li][qj], dt[j], dv, 0, 0, 0);
      dk = __builtin_amdgcn_mfma_f32_32x32x2f32(tds[w][li][qj], qt[j], dk, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kw0 + 32 * u + acc_row(r, lane);
      if (key < nk) {
        float* pv = a.dv + (krow + key) * a.lddv + h * 32 + li;
        float* pk = a.dk + (krow + key) * a.lddk + h * 32 + li;
        *pv = a.acc_kv ? *pv + dv[r] : dv[r];
        *pk = a.acc_kv ? *pk + dk[r] * a.scale : dk[r] * a.scale;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // tile reads done before the next tile's writes
  }
  f32x16 dq = dqu[0];
#pragma unroll
  for (int u = 1; u < KT; ++u) dq += dqu[u];
#pragma unroll
  for (int r = 0; r < 16; ++r) xq[w][acc_row(r, lane)][li] = dq[r];
  __syncthreads();
  const int ns = (Tv + a.Tc - 1) / a.Tc;
  {   // thread -> (query tid / 8, 4 consecutive d): one 16-B partial store (as the forward)
    const int q = tid >> 3, d0 = (tid & 7) * 4;
    float4 v;
    v.x = (xq[0][q][d0] + xq[1][q][d0]) + (xq[2][q][d0] + xq[3][q][d0]);
    v.y = (xq[0][q][d0 + 1] + xq[1][q][d0 + 1]) + (xq[2][q][d0 + 1] + xq[3][q][d0 + 1]);
    v.z = (xq[0][q][d0 + 2] + xq[1][q][d0 + 2]) + (xq[2][q][d0 + 2] + xq[3][q][d0 + 2]);
    v.w = (xq[0][q][d0 + 3] + xq[1][q][d0 + 3]) + (xq[2][q][d0 + 3] + xq[3][q][d0 + 3]);
    if (!store_partial<false>(a, vid, h, c, ns, q, d0, v, 0.f, 0.f) && q < Qn) {
      float* op = a.out + (qrow + q) * a.ld_out + h * 32 + d0;
      op[0] = v.x * a.scale;
      op[1] = v.y * a.scale;
      op[2] = v.z * a.scale;
      op[3] = v.w * a.scale;
    }
  }
  if (ns > 1 && a.cnt) fold_merge(a, vid, h, ns, false, a.scale, qrow, nullptr, nullptr);
}

}  // namespace

void attn_t_dev::launch_tattn_rr(const TAttnArgs& a, bool bwd, int KT, dim3 grid, hipStream_t s) {
  if (bwd) {
    if (KT == 2) fx_launch(tattn_bwd32_kernel<2>, grid, dim3(AT), 0, s, a);
    else fx_launch(tattn_bwd32_kernel<1>, grid, dim3(AT), 0, s, a);
  } else {
    if (KT == 2) fx_launch(tattn_fwd32_kernel<2>, grid, dim3(AT), 0, s, a);
    else fx_launch(tattn_fwd32_kernel<1>, grid, dim3(AT), 0, s, a);
  }
}

}  // namespace fx

#ifdef TATTN_STAMPS
extern "C" int fx_debug_tattn_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fx::g_ta_st), sizeof(fx::g_ta_st)) == hipSuccess ? 0 : -1;
}
#endif
