// Multi-head attention of a few queries over T frames, fused (SCALayer cross-attention,
// basic.py:508-516: nn.MultiheadAttention with Q = Nact action tokens, K/V = T frames, 8 heads): the
// LDS-staged kernel family, which takes every head dim <= 64, up to 64 queries per launch and rows of any
// alignment.  (Head dim 32 with <= 32 queries and 16-B aligned rows runs attn_t_rr.hip instead; the choice
// and the launch geometry are tattn_plan's, attention.cpp.)
//
// The reference runs the attention as ATen bmm -> softmax -> (dropout) -> bmm and keeps the (h, Q, T)
// probabilities for backward.  Here one launch covers every video and head, flash-decoding style:
//   grid = (T-chunk c, head h, video v); a workgroup stages q_h (Q x hd), K_c and V_c (Tc x hd) in
//   LDS, computes S = q K_c^T (MFMA 32x32x2 f32), its row max m_c / sum l_c, and O_c = exp(S - m_c) V_c.
//   One chunk per video: o and lse are written directly.  More: the partials go to the workspace (TAttnWs)
//   and a second, small launch (tattn_merge_kernel, one workgroup per (video, head)) merges them in chunk
//   order -- deterministic -- into o = sum_c e^(m_c - M) O_c / L and lse = M + log L.  These kernels have no
//   arrival counter; the register-resident family merges inside its launch and uses tattn_merge_kernel
//   only past FOLD_MAX chunks.
//   Only lse (Q floats per head) is kept for backward, not the probabilities.
// Backward recomputes P = exp(S - lse) per chunk: dV_c = P^T dO, dP = dO V_c^T, dS = P (dP - D)
// with D = rowsum(dO o), dK_c = scale dS^T q (K/V rows of a chunk belong to ONE workgroup: written,
// not accumulated; a later query block of the same keys adds), and dq = scale sum_c dS_c K_c through the
// same ordered merge launch.
// HBM bytes per frame and layer: K and V rows read once per query block (2 hd h x 4 B per frame forward;
// backward also writes dK, dV).
#include <cmath>
#include <mutex>

#include "attn_t_dev.h"

namespace fx {
namespace {
using namespace attn_t_dev;

// acc (32x32) += A (32 x K) . B (K x 32), operands in LDS.
//   A element (r, k) = ATR ? a[k*lda + r] : a[r*lda + k]
//   B element (k, c) = BTR ? b[c*ldb + k] : b[k*ldb + c]
// K even; lane half hh takes k in [hh*K/2, hh*K/2 + K/2) -- any k order works as long as A and B agree.
// Strides are odd (row length + 1) so the 32 lanes of a half hit 32 different banks.
template <bool ATR, bool BTR>
__device__ __forceinline__ void mm32(const float* a, int lda, const float* b, int ldb, int K, f32x16& acc, int lane) {
  // K % 8 == 0 (every caller).  Software-pipelined: the LDS reads of the next 4 k-steps are issued
  // before the MFMAs of the current 4.
  const int li = lane & 31, kh = (lane >> 5) * (K >> 1);
  float av[4], bv[4];
  auto ld4 = [&](int j0, float* x, float* y) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kh + j0 + j;
      x[j] = ATR ? a[k * lda + li] : a[li * lda + k];
      y[j] = BTR ? b[li * ldb + k] : b[k * ldb + li];
    }
  };
  ld4(0, av, bv);
  for (int j0 = 0; j0 < (K >> 1); j0 += 4) {
    float an[4], bn[4];
    if (j0 + 4 < (K >> 1)) ld4(j0 + 4, an, bn);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      av[j] = an[j];
      bv[j] = bn[j];
    }
  }
}

// The same product with A row-major (k contiguous per row) read as ds_read_b128: a lane half's k range is
// contiguous, so one 16-B read feeds 4 MFMAs.  B: BTR -> also contiguous k (b128); else b[k*ldb + c] (b32).
// lda (and ldb for BTR) = row length + 4: 16-B aligned rows, conflict-free b128 lane groups.
template <bool BTR>
__device__ __forceinline__ void mm32v(const float* a, int lda, const float* b, int ldb, int K, f32x16& acc, int lane) {
  const int li = lane & 31, kh = (lane >> 5) * (K >> 1);
  const float* pa = a + li * lda + kh;
  const float* pb = BTR ? b + li * ldb + kh : b + kh * ldb + li;
  auto ldb4 = [&](int j0) {
    if (BTR) return *reinterpret_cast<const float4*>(pb + j0);
    return make_float4(pb[j0 * ldb], pb[(j0 + 1) * ldb], pb[(j0 + 2) * ldb], pb[(j0 + 3) * ldb]);
  };
  float4 av = *reinterpret_cast<const float4*>(pa), bv = ldb4(0);
  for (int j0 = 0; j0 < (K >> 1); j0 += 4) {
    float4 an = av, bn = bv;
    if (j0 + 4 < (K >> 1)) {
      an = *reinterpret_cast<const float4*>(pa + j0 + 4);
      bn = ldb4(j0 + 4);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
    av = an;
    bv = bn;
  }
}

// Strips of row-major sources staged into LDS images (row stride ld, zero outside the `nvalid` rows and
// `hd` columns).  Every load of a workgroup's strips is issued before the first LDS store (a store
// behind its own load would serialise the strips on the memory latency): float4 loads when every row
// slice is 16-B aligned, up to NV float4 per thread and strip.
template <int NV>
struct Strip {
  float4 v[NV];
  __device__ __forceinline__ void load(int rows, int cols, const float* src, long long lds_, int nvalid, int hd,
                                       int tid) {
    const int c4 = cols >> 2, total = rows * c4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + i * AT;
      const int r = e / c4, c = (e - r * c4) * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < total && r < nvalid && c < hd) x = *reinterpret_cast<const float4*>(src + (long long)r * lds_ + c);
      v[i] = x;
    }
  }
  __device__ __forceinline__ void store(float* img, int ld, int rows, int cols, int tid) const {
    const int c4 = cols >> 2, total = rows * c4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + i * AT;
      if (e < total) {
        const int r = e / c4, c = (e - r * c4) * 4;
        float* d = img + r * ld + c;
        d[0] = v[i].x;
        d[1] = v[i].y;
        d[2] = v[i].z;
        d[3] = v[i].w;
      }
    }
  }
};
constexpr int NVQ = 4;    // q / o / dout strips: <= 64 x 64 floats
// (K / V chunks: NVK float4, <= 8192 floats -- tattn_plan keeps Tc * Hp within it)

// element-wise fallback for unaligned / odd-width slices
__device__ __forceinline__ void stage_scalar(float* img, int ld, int rows, int cols, const float* src, long long lds_,
                                             int nvalid, int hd, int tid) {
  for (int e = tid; e < rows * cols; e += AT) {
    const int r = e / cols, c = e - r * cols;
    img[r * ld + c] = (r < nvalid && c < hd) ? src[(long long)r * lds_ + c] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------ forward
// grid (chunk, head, video).  nsplit == 1: o and lse directly; else the chunk's partial
// O_c = e^(S - m_c) V_c (Qp x Hp) and its row stats (m_c, l_c) go to the workspace for tattn_merge_kernel.
__global__ __launch_bounds__(AT) void tattn_fwd_kernel(TAttnArgs a) {
  extern __shared__ float sm[];
  const int c = blockIdx.x, h = blockIdx.y, vid = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Qp = a.Qp, Hp = a.Hp, Tc = a.Tc, hd = a.hd;
  const int lq = Hp + 4, lk = Hp + 4, ls = Tc + 4;   // 16-B aligned rows (b128 operand reads)
  float* qs = sm;                       // [Qp][lq]
  float* ks = qs + Qp * lq;             // [Tc][lk]
  float* vs = ks + Tc * lk;             // [Tc][lk]
  float* ss = vs + Tc * lk;             // [Qp][ls]
  float* red = ss + Qp * ls;            // [4][1024] wave partials
  float* rowm = red + 4 * 1024;         // [Qp]
  float* rowl = rowm + Qp;              // [Qp]
  const auto [Tv, t0, nk, Qn, qrow, krow] = tattn_chunk(a, c, vid);
  if (nk <= 0 || Qn <= 0) return;   // (a short video has no query in this block; no arrival: the merge is a launch)
  const float* qsrc = a.q + qrow * a.ldq + h * hd;
  const float* ksrc = a.k + krow * a.ldk + h * hd;
  const float* vsrc = a.v + krow * a.ldv + h * hd;
  if (a.vec) {
    Strip<NVQ> sq;
    Strip<NVK> sk, sv;
    sq.load(Qp, Hp, qsrc, a.ldq, Qn, hd, tid);
    sk.load(Tc, Hp, ksrc, a.ldk, nk, hd, tid);
    sv.load(Tc, Hp, vsrc, a.ldv, nk, hd, tid);
    sq.store(qs, lq, Qp, Hp, tid);
    sk.store(ks, lk, Tc, Hp, tid);
    sv.store(vs, lk, Tc, Hp, tid);
  } else {
    stage_scalar(qs, lq, Qp, Hp, qsrc, a.ldq, Qn, hd, tid);
    stage_scalar(ks, lk, Tc, Hp, ksrc, a.ldk, nk, hd, tid);
    stage_scalar(vs, lk, Tc, Hp, vsrc, a.ldv, nk, hd, tid);
  }
  __syncthreads();
  // S^T tiles (keys x queries) = scale K q^T kept in registers: wave w takes tiles w and w + 4 of the
  // (key tile, query tile) grid -- both in query tile w % nrt -- and a lane holds 16 keys of ONE query
  // column, so the softmax statistics are in-register reductions, one exchange with the other lane
  // half and one pass through LDS across the waves.  Keys past the video: -inf.
  const int nrt = Qp / 32, nct = Tc / 32;
  const int qtw = wave % nrt;
  const int myq = qtw * 32 + (lane & 31);
  f32x16 st[2];
  bool has[2];
  float lm = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = wave + 4 * u;
    has[u] = t < nrt * nct;
    zero16(st[u]);
    if (has[u]) {
      const int kt = t / nrt;
      mm32v<true>(ks + kt * 32 * lk, lk, qs + qtw * 32 * lq, lq, Hp, st[u], lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + acc_row(r, lane);
        st[u][r] = key < nk ? st[u][r] * a.scale : -INFINITY;
        lm = fmaxf(lm, st[u][r]);
      }
    }
  }
  float* wmax = red;              // [4][Qp]: per-wave maxima (-inf where the wave has no keys of a query)
  float* wsum = red + 4 * Qp;     // [4][Qp]: per-wave sums
  lm = fmaxf(lm, __shfl_xor(lm, 32, 64));
  if (lane < Qp) wmax[wave * Qp + lane] = (has[0] && (lane >> 5) == qtw) ? lm : -INFINITY;
  __syncthreads();
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) M = fmaxf(M, wmax[w * Qp + myq]);
  float ls_ = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!has[u]) continue;
    const int kt = (wave + 4 * u) / nrt;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __expf(st[u][r] - M);
      ls_ += p;                                          // the softmax normaliser sees every key
      const int key = kt * 32 + acc_row(r, lane);
      const float kp = (a.drop_p > 0.f && key < nk) ? drop_keep(a, qrow + myq, h, krow + key) : 1.f;
      ss[myq * ls + key] = p * kp;                       // (dropped) P image [query][key] for P V
    }
  }
  ls_ += __shfl_xor(ls_, 32, 64);
  if (lane < Qp) wsum[wave * Qp + lane] = (has[0] && (lane >> 5) == qtw) ? ls_ : 0.f;
  __syncthreads();
  if (wave < nrt && lane < 32) {
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += wsum[w * Qp + myq];
    rowm[myq] = M;
    rowl[myq] = L;
  }
  __syncthreads();
  // O_c = P V: nt output tiles, each split over wpt waves along the chunk
  const int nht = Hp / 32, nt = nrt * nht, wpt = 4 / nt;
  const int tile = wave / wpt, part = wave - tile * wpt;
  const int dlen = Tc / wpt, d0 = part * dlen;
  const int rt = tile / nht, ht = tile - rt * nht;
  f32x16 acc;
  zero16(acc);
  mm32v<false>(ss + rt * 32 * ls + d0, ls, vs + d0 * lk + ht * 32, lk, dlen, acc, lane);
  if (wpt > 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[r];
    __syncthreads();
    if (part == 0)
      for (int q = 1; q < wpt; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[(wave + q) * 1024 + r * 64 + lane];
  }
  const TAttnWs W(gridDim.z, a.nh, a.nsplit, Qp, Hp);
  const long long pid = TAttnWs::pid(vid, a.nh, h, a.nsplit, c);
  if (part == 0) {
    const int col = ht * 32 + (lane & 31);
    if (a.nsplit == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rt * 32 + acc_row(r, lane);
        if (row < Qn && col < hd) a.out[(qrow + row) * a.ld_out + h * hd + col] = acc[r] / rowl[row];
      }
    } else {
      float* po = a.ws + W.tile(pid);
#pragma unroll
      for (int r = 0; r < 16; ++r) po[(rt * 32 + acc_row(r, lane)) * Hp + col] = acc[r];
    }
  }
  if (a.nsplit == 1) {
    for (int r = tid; r < Qn; r += AT)
      a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + r] = rowm[r] + __logf(rowl[r]);
    return;
  }
  float* pm = a.ws + W.m();
  float* pl = a.ws + W.l();
  for (int r = tid; r < Qp; r += AT) {
    pm[pid * Qp + r] = rowm[r];
    pl[pid * Qp + r] = rowl[r];
  }
}

// Ordered merge of the nsplit partials of one (video, head) per workgroup, chunk order fixed
// (deterministic).  Forward (stats != 0): w_s(r) = e^(m_s - M) / L, o = sum_s w_s O_s, lse = M + log L;
// backward: dq = scale * sum_s dq_s.  A thread owns 4 consecutive columns of a row with 16 splits'
// float4 loads in flight.  grid (head, video).
__global__ __launch_bounds__(AT) void tattn_merge_kernel(TAttnArgs a, int stats, float mul) {
  extern __shared__ float sm[];
  const int h = blockIdx.x, vid = blockIdx.y, nvid = gridDim.y, tid = threadIdx.x;
  const int Qp = a.Qp, Hp = a.Hp, hd = a.hd, nsm = a.nsplit;
  const int Qn = live_queries(a, vid);
  if (Qn <= 0) return;                   // (the block's workgroups of this video left no partials)
  const int ns = (a.koff[vid + 1] - a.koff[vid] + a.Tc - 1) / a.Tc;   // this video's chunks
  const TAttnWs W(nvid, a.nh, nsm, Qp, Hp);
  const long long pbase = TAttnWs::pid(vid, a.nh, h, nsm, 0);
  const float* part = a.ws + W.tile(pbase);
  float* w = sm;                         // [ns][Qp] weights
  float* wl = sm + ns * Qp;              // [ns][Qp] l partials
  if (stats) {
    const float* pm = a.ws + W.m() + pbase * Qp;
    const float* pl = a.ws + W.l() + pbase * Qp;
    for (int e = tid; e < ns * Qp; e += AT) {
      w[e] = pm[e];
      wl[e] = pl[e];
    }
    __syncthreads();
    for (int r = tid; r < Qp; r += AT) {
      float M = -INFINITY;
      for (int sp = 0; sp < ns; ++sp) M = fmaxf(M, w[sp * Qp + r]);
      float L = 0.f;
      for (int sp = 0; sp < ns; ++sp) L += __expf(w[sp * Qp + r] - M) * wl[sp * Qp + r];
      const float inv = 1.f / L;
      for (int sp = 0; sp < ns; ++sp) w[sp * Qp + r] = __expf(w[sp * Qp + r] - M) * inv;
      if (r < Qn) a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + r] = M + __logf(L);
    }
    __syncthreads();
  }
  float* out = a.out + ((long long)a.qoff[vid] + a.q0) * a.ld_out + h * hd;
  const int c4 = Hp >> 2;
  for (int e = tid; e < Qn * c4; e += AT) {
    const int r = e / c4, col = (e - r * c4) * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < ns; s0 += 16) {
      float4 x[16];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        x[j] = *reinterpret_cast<const float4*>(part + ((long long)min(s0 + j, ns - 1) * Qp + r) * Hp + col);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (s0 + j < ns) {
          const float ww = stats ? w[(s0 + j) * Qp + r] : 1.f;
          acc.x += ww * x[j].x;
          acc.y += ww * x[j].y;
          acc.z += ww * x[j].z;
          acc.w += ww * x[j].w;
        }
      }
    }
    float* o = out + (long long)r * a.ld_out + col;
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col + j < hd) o[j] = v[j] * mul;
  }
}

// ------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(AT) void tattn_bwd_kernel(TAttnArgs a) {
  extern __shared__ float sm[];
  const int c = blockIdx.x, h = blockIdx.y, vid = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Qp = a.Qp, Hp = a.Hp, Tc = a.Tc, hd = a.hd;
  const int lq = Hp + 4, ls = Tc + 4;   // 16-B aligned rows (b128 operand reads)
  float* qs = sm;                       // [Qp][lq]
  float* dos = qs + Qp * lq;            // [Qp][lq]
  float* ks = dos + Qp * lq;            // [Tc][lq]
  float* vs = ks + Tc * lq;             // [Tc][lq]
  float* ps = vs + Tc * lq;             // [Qp][ls]  P   (o until P is written)
  float* ds = ps + Qp * ls;             // [Qp][ls]  dS
  float* red = ds + Qp * ls;            // [4][1024]
  float* rl = red + 4 * 1024;           // [Qp] lse
  float* rd = rl + Qp;                  // [Qp] D
  const auto [Tv, t0, nk, Qn, qrow, krow] = tattn_chunk(a, c, vid);
  if (nk <= 0 || Qn <= 0) return;   // (a short video has no query in this block; no arrival: the merge is a launch)
  const float* qsrc = a.q + qrow * a.ldq + h * hd;
  const float* dsrc = a.dout + qrow * a.lddo + h * hd;
  const float* osrc = a.o + qrow * a.ldo + h * hd;
  const float* ksrc = a.k + krow * a.ldk + h * hd;
  const float* vsrc = a.v + krow * a.ldv + h * hd;
  if (tid < Qp) rl[tid] = tid < Qn ? a.lse[((long long)vid * a.nh + h) * a.qs + a.q0 + tid] : 0.f;
  if (a.vec) {
    Strip<NVQ> sq, sd, so;
    Strip<NVK> sk, sv;
    sq.load(Qp, Hp, qsrc, a.ldq, Qn, hd, tid);
    sd.load(Qp, Hp, dsrc, a.lddo, Qn, hd, tid);
    so.load(Qp, Hp, osrc, a.ldo, Qn, hd, tid);
    sk.load(Tc, Hp, ksrc, a.ldk, nk, hd, tid);
    sv.load(Tc, Hp, vsrc, a.ldv, nk, hd, tid);
    sq.store(qs, lq, Qp, Hp, tid);
    sd.store(dos, lq, Qp, Hp, tid);
    so.store(ps, lq, Qp, Hp, tid);
    sk.store(ks, lq, Tc, Hp, tid);
    sv.store(vs, lq, Tc, Hp, tid);
  } else {
    stage_scalar(qs, lq, Qp, Hp, qsrc, a.ldq, Qn, hd, tid);
    stage_scalar(dos, lq, Qp, Hp, dsrc, a.lddo, Qn, hd, tid);
    stage_scalar(ps, lq, Qp, Hp, osrc, a.ldo, Qn, hd, tid);
    stage_scalar(ks, lq, Tc, Hp, ksrc, a.ldk, nk, hd, tid);
    stage_scalar(vs, lq, Tc, Hp, vsrc, a.ldv, nk, hd, tid);
  }
  __syncthreads();
  // D_i = sum_d dO_id o_id
  if (tid < Qp) {
    float d = 0.f;
    for (int j = 0; j < Hp; ++j) d += dos[tid * lq + j] * ps[tid * lq + j];
    rd[tid] = d;
  }
  __syncthreads();
  const int nrt = Qp / 32, nct = Tc / 32, nht = Hp / 32;
  // P = exp(scale q K^T - lse) and dS = P (dO V^T - D), tile by tile
  for (int t = wave; t < nrt * nct; t += 4) {
    const int rt = t / nct, ct = t - rt * nct;
    f32x16 s, dp;
    zero16(s);
    zero16(dp);
    mm32v<true>(qs + rt * 32 * lq, lq, ks + ct * 32 * lq, lq, Hp, s, lane);
    mm32v<true>(dos + rt * 32 * lq, lq, vs + ct * 32 * lq, lq, Hp, dp, lane);
    const int col = ct * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rt * 32 + acc_row(r, lane);
      const float p = (col < nk && row < Qn) ? __expf(s[r] * a.scale - rl[row]) : 0.f;
      // dropout: P_d = P keep / (1-p) multiplies V; dP = (dO V^T) keep / (1-p); D = rowsum(dO o) still
      const float kp = (a.drop_p > 0.f && p != 0.f) ? drop_keep(a, qrow + row, h, krow + col) : 1.f;
      ps[row * ls + col] = p * kp;
      ds[row * ls + col] = p * (dp[r] * kp - rd[row]);
    }
  }
  __syncthreads();
  // dV_c = P^T dO and dK_c = scale dS^T q  (Tc x Hp each), written straight to their rows
  for (int t = wave; t < 2 * nct * nht; t += 4) {
    const int which = t / (nct * nht), u = t - which * nct * nht;
    const int kt = u / nht, ht = u - kt * nht;
    f32x16 acc;
    zero16(acc);
    if (which == 0)
      mm32<true, false>(ps + kt * 32, ls, dos + ht * 32, lq, Qp, acc, lane);
    else
      mm32<true, false>(ds + kt * 32, ls, qs + ht * 32, lq, Qp, acc, lane);
    const int col = ht * 32 + (lane & 31);
    float* dst = which == 0 ? a.dv : a.dk;
    const long long ld = which == 0 ? a.lddv : a.lddk;
    const float mul = which == 0 ? 1.f : a.scale;
    if (col < hd) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + acc_row(r, lane);
        if (key < nk) {
          float* d = dst + (krow + key) * ld + h * hd + col;
          *d = a.acc_kv ? *d + acc[r] * mul : acc[r] * mul;
        }
      }
    }
  }
  // dq partial = dS K_c  (Qp x Hp), tiles split along the chunk like the forward's O
  const int nt = nrt * nht, wpt = 4 / nt;
  const int tile = wave / wpt, part = wave - tile * wpt;
  const int dlen = Tc / wpt, d0 = part * dlen;
  const int rt = tile / nht, ht = tile - rt * nht;
  f32x16 acc;
  zero16(acc);
  mm32v<false>(ds + rt * 32 * ls + d0, ls, ks + d0 * lq + ht * 32, lq, dlen, acc, lane);
  if (wpt > 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[r];
    __syncthreads();
    if (part == 0)
      for (int q = 1; q < wpt; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[(wave + q) * 1024 + r * 64 + lane];
  }
  if (part == 0) {
    const int col = ht * 32 + (lane & 31);
    if (a.nsplit == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rt * 32 + acc_row(r, lane);
        if (row < Qn && col < hd) a.out[(qrow + row) * a.ld_out + h * hd + col] = acc[r] * a.scale;
      }
    } else {
      float* po = a.ws + TAttnWs(gridDim.z, a.nh, a.nsplit, Qp, Hp).tile(TAttnWs::pid(vid, a.nh, h, a.nsplit, c));
#pragma unroll
      for (int r = 0; r < 16; ++r) po[(rt * 32 + acc_row(r, lane)) * Hp + col] = acc[r];
    }
  }
}

// dynamic LDS above the 64 KB default (gfx950: 160 KB per workgroup)
void lds_setup() {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)tattn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)tattn_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)tattn_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
}

}  // namespace

void attn_t_dev::launch_tattn_lds(const TAttnArgs& a, bool bwd, dim3 grid, size_t lds, hipStream_t s) {
  lds_setup();
  if (bwd) fx_launch(tattn_bwd_kernel, grid, dim3(AT), lds, s, a);
  else fx_launch(tattn_fwd_kernel, grid, dim3(AT), lds, s, a);
}

void attn_t_dev::launch_tattn_merge(const TAttnArgs& a, int nvid, bool stats, float mul, size_t lds, hipStream_t s) {
  lds_setup();
  fx_launch(tattn_merge_kernel, dim3(a.nh, nvid), dim3(AT), lds, s, a, (int)stats, mul);
}

}  // namespace fx
