// Factorised loss terms and prediction of the verb/noun FACT (fact_clip/models/blocks_SepVerbNoun.py
// with loss.py): every action log-probability is
//   logp[r, a] = lsv[r, vids[a]] + lsn[r, nids[a]]      (lsv / lsn: log-softmax of the verb / noun heads)
// so each term is computed from the n1 + n2 head values of a row staged in LDS, as verbnoun.hip stages
// them; the rows x A table is never built.
//   vn_loss fwd/bwd : frame_loss (loss.py:246-258) and Block.action_token_loss
//                     (blocks_SepVerbNoun.py:271-283) with hard labels, frame_loss_tdu (260-277) with the
//                     frame labels of each TDU segment, smooth_loss (8-18) over consecutive rows
//   vn_eval_pred    : Block._eval (blocks_SepVerbNoun.py:323-342)
//   vn_terms fwd/bwd: the same loss rows as FX_TERM_VNCLASS terms of the loss term table (vloss.hip):
//                     workgroup b of a term takes rows b, b + FX_LOSS_NB, ... in ascending order
//   vn_match_cost   : MatchCriterion.match's cost (loss.py:108-153, soft IoU 91-106) from the token heads
//                     and interval overlaps of the (segment-level) attention, no T x Q x G cube
//   *_batch         : vn_match_cost / vn_eval_pred for every video of a batch (fx_vn_video descriptors): the
//                     same row code as the single-video kernels over a (row, video) grid
// Layout: one 256-thread workgroup per row (frame, segment or token).
// Determinism: no float atomics.  Reductions are wave shuffles in a fixed tree plus a fixed-order
// combine of the 4 wave partials; per-row partial sums are added by one workgroup in a fixed order;
// the backward's scatters are gathers (the VerbNounMap CSR lists for actions -> bins, a chunked
// ascending loop for a segment's frames -> bins) -- bitwise repeatable run to run.
#include <algorithm>
#include <cmath>

#include "fx_common.h"

namespace fx {
namespace {

constexpr int VL_MAXH = 2048;       // n1 + n2 head columns staged per row
constexpr int VL_THREADS = 256;
constexpr int VL_MAXLDS = 60 * 1024;   // dynamic LDS of one workgroup

__device__ inline float vl_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline float vl_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// block-wide max / sum of one value per thread: wave tree, then the 4 partials in fixed order
__device__ inline float vl_block_max(float v, float* part) {
  v = vl_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}
__device__ inline float vl_block_sum(float v, float* part) {
  v = vl_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}
// first maximum of (value, index) pairs over the workgroup; index 0x7fffffff = none
__device__ inline void vl_block_argmax(float& v, int& i, float* pv, int* pi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    pv[threadIdx.x >> 6] = v;
    pi[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = pv[0];
  i = pi[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (pv[k] > v || (pv[k] == v && pi[k] < i)) {
      v = pv[k];
      i = pi[k];
    }
}

__device__ inline float vl_block_lse(const float* sh, int n, float* part) {
  float m = -INFINITY;
  for (int c = threadIdx.x; c < n; c += VL_THREADS) m = fmaxf(m, sh[c]);
  m = vl_block_max(m, part);
  float s = 0.f;
  for (int c = threadIdx.x; c < n; c += VL_THREADS) s += expf(sh[c] - m);
  s = vl_block_sum(s, part);
  return m + logf(s);
}

// sh[0, n1 + n2) = log-softmax of both groups of the row at cr (the same arithmetic as vn_logp_fwd_kernel)
__device__ inline void vl_stage_row(const float* cr, int n1, int n2, float* sh, float* part, float* lv_out,
                                    float* ln_out) {
  const int n = n1 + n2;
  __syncthreads();
  for (int c = threadIdx.x; c < n; c += VL_THREADS) sh[c] = cr[c];
  __syncthreads();
  const float lv = vl_block_lse(sh, n1, part);
  const float ln = vl_block_lse(sh + n1, n2, part);
  __syncthreads();
  for (int c = threadIdx.x; c < n; c += VL_THREADS) sh[c] -= (c < n1 ? lv : ln);
  __syncthreads();
  *lv_out = lv;
  *ln_out = ln;
}
// the same from saved log-sum-exps
__device__ inline void vl_stage_row_lse(const float* cr, int n1, int n2, float lv, float ln, float* sh) {
  for (int c = threadIdx.x; c < n1 + n2; c += VL_THREADS) sh[c] = cr[c] - (c < n1 ? lv : ln);
}

// label y -> its verb / noun head columns and class weight (y == A with null heads: the two null bins)
__device__ inline void vl_label(long long y, const int32_t* vids, const int32_t* nids, int A, int null, int n1,
                                int n2, const float* w, int* v, int* k, float* wy) {
  const int yy = (int)min(max(y, 0LL), (long long)(A + null - 1));
  if (yy == A) {
    *v = n1 - 1;
    *k = n2 - 1;
  } else {
    *v = min(max(vids[yy], 0), n1 - 1);
    *k = min(max(nids[yy], 0), n2 - 1);
  }
  *wy = w[yy];
}

struct VnLossArgs {
  const float* clogit;   // (R, n1 + n2), leading stride ld
  long long ld;
  int R, n1, n2, A, null;
  const int32_t* vids;
  const int32_t* nids;
  const long long* y;    // hard: (R) labels; segment: (ny) frame labels; null (and y32 null): no CE term
  const int32_t* y32;    // the same labels as int32 (the term table's form); used when y is null
  int ny;
  const int32_t* seg_start;   // segment mode: (R) first / last frame of each row's segment
  const int32_t* seg_end;
  const float* w;        // (A + null) class weights
  int smooth;
};

__device__ inline bool vl_has_y(const VnLossArgs& a) { return a.y || a.y32; }
__device__ inline long long vl_y(const VnLossArgs& a, int i) { return a.y ? a.y[i] : (long long)a.y32[i]; }

// row r of the loss: its two log-sum-exps go to lse[2 r], lse[2 r + 1]; *ce = CE term of the row, *sm =
// sum_a min(d[r, a]^2, 16) (both valid on thread 0).  sh0 / sh1: VL_MAXH floats of LDS each
__device__ inline void vl_fwd_row(const VnLossArgs& a, int r, float* sh0, float* sh1, float* part, float* lse,
                                  float* ce_out, float* sm_out) {
  const int tid = threadIdx.x;
  const int n1 = a.n1, n2 = a.n2;
  float lv, ln;
  vl_stage_row(a.clogit + (long long)r * a.ld, n1, n2, sh0, part, &lv, &ln);
  if (tid == 0) {
    lse[2 * (long long)r] = lv;
    lse[2 * (long long)r + 1] = ln;
  }
  float ce = 0.f;
  if (vl_has_y(a) && !a.seg_start) {
    if (tid == 0) {
      int v, k;
      float wy;
      vl_label(vl_y(a, r), a.vids, a.nids, a.A, a.null, n1, n2, a.w, &v, &k, &wy);
      ce = -wy * (sh0[v] + sh0[n1 + k]);
    }
  } else if (vl_has_y(a)) {
    const int s0 = min(max(a.seg_start[r], 0), a.ny - 1), e0 = min(max(a.seg_end[r], s0), a.ny - 1);
    float t = 0.f;
    for (int f = s0 + tid; f <= e0; f += VL_THREADS) {
      int v, k;
      float wy;
      vl_label(vl_y(a, f), a.vids, a.nids, a.A, a.null, n1, n2, a.w, &v, &k, &wy);
      t += -wy * (sh0[v] + sh0[n1 + k]);
    }
    ce = vl_block_sum(t, part) / (float)(e0 - s0 + 1);
  }
  float sm = 0.f;
  if (a.smooth && r + 1 < a.R) {
    float l1, l2;
    vl_stage_row(a.clogit + (long long)(r + 1) * a.ld, n1, n2, sh1, part, &l1, &l2);
    float t = 0.f;
    for (int c = tid; c < a.A; c += VL_THREADS) {
      const int v = min(max(a.vids[c], 0), n1 - 1), k = n1 + min(max(a.nids[c], 0), n2 - 1);
      const float d = (sh1[v] - sh0[v]) + (sh1[k] - sh0[k]);
      t += fminf(d * d, 16.f);
    }
    sm = vl_block_sum(t, part);
  }
  *ce_out = ce;
  *sm_out = sm;
}

// part[2 r] = CE term of row r, part[2 r + 1] = sum_a min(d[r, a]^2, 16); lse (R, 2) saved
__global__ __launch_bounds__(VL_THREADS) void vn_loss_fwd_kernel(VnLossArgs a, float* lse, float* partial) {
  __shared__ float sh0[VL_MAXH];
  __shared__ float sh1[VL_MAXH];
  __shared__ float part[4];
  const int r = blockIdx.x;
  float ce, sm;
  vl_fwd_row(a, r, sh0, sh1, part, lse, &ce, &sm);
  if (threadIdx.x == 0) {
    partial[2 * (long long)r] = ce;
    partial[2 * (long long)r + 1] = sm;
  }
}

// out[0] = c0 * sum(part[2i]) + c1 * sum(part[2i+1]): every thread adds its rows in ascending order,
// then the fixed tree (c1 == 0 drops the smooth term)
__global__ __launch_bounds__(VL_THREADS) void vn_loss_finish_kernel(const float* partial, int n, float c0, float c1,
                                                                    float* out) {
  __shared__ float part[4];
  float x = 0.f, y = 0.f;
  for (int i = threadIdx.x; i < n; i += VL_THREADS) {
    x += partial[2 * (long long)i];
    y += partial[2 * (long long)i + 1];
  }
  x = vl_block_sum(x, part);
  y = vl_block_sum(y, part);
  if (threadIdx.x == 0) out[0] = c1 != 0.f ? c0 * x + c1 * y : c0 * x;
}

// the CSR inverse lists of the mapping and the LDS chunk tables of a segment's frames (VL_THREADS each)
struct VnBwdTabs {
  const int32_t* voff;
  const int32_t* vlist;
  const int32_t* noff;
  const int32_t* nlist;
  float* part;
  int* cv;
  int* ck;
  float* cw;
};

// dr[0, n) = dclogit[r, :] of g_ce * CE + g_sm * smooth.  dyn (LDS): cur[n] acc[n], and with the smooth term
// prv[n] nxt[n] ga[A] (the row's A action gradients live in LDS only).  Ends behind a barrier: the caller
// may go on to another row
__device__ inline void vl_bwd_row(const VnLossArgs& a, int r, const float* lse, float g_ce, float g_sm,
                                  const VnBwdTabs& tb, float* dyn, float* dr) {
  const int32_t *voff = tb.voff, *vlist = tb.vlist, *noff = tb.noff, *nlist = tb.nlist;
  float* part = tb.part;
  int *cv = tb.cv, *ck = tb.ck;
  float* cw = tb.cw;
  const int tid = threadIdx.x;
  const int n1 = a.n1, n2 = a.n2, n = n1 + n2;
  float* cur = dyn;
  float* acc = dyn + n;
  vl_stage_row_lse(a.clogit + (long long)r * a.ld, n1, n2, lse[2 * (long long)r], lse[2 * (long long)r + 1], cur);
  for (int j = tid; j < n; j += VL_THREADS) acc[j] = 0.f;
  __syncthreads();
  if (vl_has_y(a) && !a.seg_start) {
    int v, k;
    float wy;
    vl_label(vl_y(a, r), a.vids, a.nids, a.A, a.null, n1, n2, a.w, &v, &k, &wy);
    for (int j = tid; j < n; j += VL_THREADS)
      acc[j] = (g_ce * wy) * (expf(cur[j]) - ((j == v || j == n1 + k) ? 1.f : 0.f));
  } else if (vl_has_y(a)) {
    const int s0 = min(max(a.seg_start[r], 0), a.ny - 1), e0 = min(max(a.seg_end[r], s0), a.ny - 1);
    float wtot = 0.f;
    for (int base = s0; base <= e0; base += VL_THREADS) {   // the segment's frames in ascending chunks
      const int cnt = min(VL_THREADS, e0 - base + 1);
      __syncthreads();
      if (tid < cnt) {
        int v, k;
        float wy;
        vl_label(vl_y(a, base + tid), a.vids, a.nids, a.A, a.null, n1, n2, a.w, &v, &k, &wy);
        cv[tid] = v;
        ck[tid] = n1 + k;
        cw[tid] = wy;
        wtot += wy;
      }
      __syncthreads();
      for (int j = tid; j < n; j += VL_THREADS) {   // every bin adds its frames of the chunk in ascending order
        const int* cb = j < n1 ? cv : ck;
        float s = acc[j];
        for (int i = 0; i < cnt; ++i)
          if (cb[i] == j) s += cw[i];
        acc[j] = s;
      }
    }
    wtot = vl_block_sum(wtot, part);
    const float gl = g_ce / (float)(e0 - s0 + 1);
    for (int j = tid; j < n; j += VL_THREADS) acc[j] = gl * (wtot * expf(cur[j]) - acc[j]);
  }
  if (a.smooth) {
    float* prv = dyn + 2 * n;
    float* nxt = dyn + 3 * n;
    float* ga = dyn + 4 * n;
    const bool hp = r > 0, hn = r + 1 < a.R;
    if (hp)
      vl_stage_row_lse(a.clogit + (long long)(r - 1) * a.ld, n1, n2, lse[2 * (long long)(r - 1)],
                       lse[2 * (long long)(r - 1) + 1], prv);
    if (hn)
      vl_stage_row_lse(a.clogit + (long long)(r + 1) * a.ld, n1, n2, lse[2 * (long long)(r + 1)],
                       lse[2 * (long long)(r + 1) + 1], nxt);
    __syncthreads();
    float tot = 0.f;
    for (int c = tid; c < a.A; c += VL_THREADS) {
      const int v = min(max(a.vids[c], 0), n1 - 1), k = n1 + min(max(a.nids[c], 0), n2 - 1);
      float g = 0.f;
      if (hp) {
        const float d = (cur[v] - prv[v]) + (cur[k] - prv[k]);
        if (d * d <= 16.f) g += 2.f * d;
      }
      if (hn) {
        const float d = (nxt[v] - cur[v]) + (nxt[k] - cur[k]);
        if (d * d <= 16.f) g -= 2.f * d;
      }
      g *= g_sm;
      ga[c] = g;
      tot += g;
    }
    tot = vl_block_sum(tot, part);   // (its barriers also publish ga)
    for (int j = tid; j < n; j += VL_THREADS) {
      const bool verb = j < n1;
      const int b = verb ? j : j - n1;
      const int32_t* off = verb ? voff : noff;
      const int32_t* lst = verb ? vlist : nlist;
      float s = 0.f;
      const int e = min(off[b + 1], a.A);
      for (int i = max(off[b], 0); i < e; ++i) s += ga[min(max(lst[i], 0), a.A - 1)];
      acc[j] += s - expf(cur[j]) * tot;
    }
  }
  for (int j = tid; j < n; j += VL_THREADS) dr[j] = acc[j];   // (each thread reads back its own slots)
  __syncthreads();
}

__global__ __launch_bounds__(VL_THREADS) void vn_loss_bwd_kernel(VnLossArgs a, const float* lse, const float* gout,
                                                                 float c_ce, float c_sm, const int32_t* voff,
                                                                 const int32_t* vlist, const int32_t* noff,
                                                                 const int32_t* nlist, float* dcl, long long lddc) {
  extern __shared__ float dyn[];
  __shared__ float part[4];
  __shared__ int cv[VL_THREADS], ck[VL_THREADS];
  __shared__ float cw[VL_THREADS];
  const int r = blockIdx.x;
  const VnBwdTabs tb{voff, vlist, noff, nlist, part, cv, ck, cw};
  vl_bwd_row(a, r, lse, gout[0] * c_ce, gout[0] * c_sm, tb, dyn, dcl + (long long)r * lddc);
}

// ---------------------------------------------------------------- the term table's VNCLASS terms
__device__ inline VnLossArgs vl_term_args(const fx_loss_term& t, const fx_vn_term& m) {
  VnLossArgs a;
  a.clogit = t.x;
  a.ld = t.sr;
  a.R = t.R;
  a.n1 = m.n1;
  a.n2 = m.n2;
  a.A = m.A;
  a.null = m.null ? 1 : 0;
  a.vids = m.vids;
  a.nids = m.nids;
  a.y = nullptr;
  a.y32 = t.y;
  a.ny = t.rs ? t.D : t.R;
  a.seg_start = t.rs;
  a.seg_end = t.re;
  a.w = t.w;
  a.smooth = t.c_sm != 0.f;
  return a;
}

// grid (FX_LOSS_NB, nterms): workgroup b of a VNCLASS term adds its rows b, b + FX_LOSS_NB, ... in ascending
// order into the two partials terms_finish_kernel sums
__global__ __launch_bounds__(VL_THREADS) void vn_terms_fwd_kernel(const fx_loss_term* terms, float* partial) {
  __shared__ float sh0[VL_MAXH];
  __shared__ float sh1[VL_MAXH];
  __shared__ float part[4];
  const fx_loss_term& t = terms[blockIdx.y];
  if (t.kind != FX_TERM_VNCLASS) return;
  const VnLossArgs a = vl_term_args(t, *t.vn);
  float ce = 0.f, sm = 0.f;
  for (int r = blockIdx.x; r < a.R; r += gridDim.x) {
    float c, s;
    vl_fwd_row(a, r, sh0, sh1, part, t.lse, &c, &s);
    ce += c;
    sm += s;
  }
  if (threadIdx.x == 0) {
    partial[(t.slot * (long long)gridDim.x + blockIdx.x) * 2] = ce;
    partial[(t.slot * (long long)gridDim.x + blockIdx.x) * 2 + 1] = sm;
  }
}

__global__ __launch_bounds__(VL_THREADS) void vn_terms_bwd_kernel(const fx_loss_term* terms, const float* gterm) {
  extern __shared__ float dyn[];
  __shared__ float part[4];
  __shared__ int cv[VL_THREADS], ck[VL_THREADS];
  __shared__ float cw[VL_THREADS];
  const fx_loss_term& t = terms[blockIdx.y];
  if (t.kind != FX_TERM_VNCLASS) return;
  const fx_vn_term& m = *t.vn;
  const VnLossArgs a = vl_term_args(t, m);
  const VnBwdTabs tb{m.voff, m.vlist, m.noff, m.nlist, part, cv, ck, cw};
  const float g = gterm[blockIdx.y];
  for (int r = blockIdx.x; r < a.R; r += gridDim.x)
    vl_bwd_row(a, r, t.lse, g * t.c_ce, g * t.c_sm, tb, dyn, t.dx + (long long)r * t.dsr);
}

// ---------------------------------------------------------------- prediction
// per token q: ws row q = log-softmax of the n1 + 1 / n2 + 1 token heads, then Z_q = sum_a exp(logp[q, a])
// and is_tok (the null column is not the first maximum over the A + 1 columns)
__device__ inline void vl_eval_tok_row(const float* arow, int n1, int n2, const int32_t* vids, const int32_t* nids,
                                       int A, float* wr, float* sh, float* part) {
  const int tid = threadIdx.x;
  const int m1 = n1 + 1, m2 = n2 + 1, m = m1 + m2;
  float lv, ln;
  vl_stage_row(arow, m1, m2, sh, part, &lv, &ln);
  float z = 0.f, best = -INFINITY;
  for (int c = tid; c < A; c += VL_THREADS) {
    const int v = min(max(vids[c], 0), n1 - 1), k = min(max(nids[c], 0), n2 - 1);
    const float lp = sh[v] + sh[m1 + k];
    z += expf(lp);
    best = fmaxf(best, lp);
  }
  z = vl_block_sum(z, part);
  best = vl_block_max(best, part);
  for (int c = tid; c < m; c += VL_THREADS) wr[c] = sh[c];
  if (tid == 0) {
    wr[m] = z;
    wr[m + 1] = (sh[m1 - 1] + sh[m - 1]) > best ? 0.f : 1.f;
  }
}

__global__ __launch_bounds__(VL_THREADS) void vn_eval_tok_kernel(const float* aclogit, long long lda, int n1, int n2,
                                                                 const int32_t* vids, const int32_t* nids, int A,
                                                                 float* ws, int wld) {
  __shared__ float sh[VL_MAXH];
  __shared__ float part[4];
  const int q = blockIdx.x;
  vl_eval_tok_row(aclogit + (long long)q * lda, n1, n2, vids, nids, A, ws + (long long)q * wld, sh, part);
}

// per frame t: the first maximum of its attention over the non-null tokens, then the first maximum over a
// of (1 - w) exp(logp_q[tok, a]) / Z_tok + w exp(logp_f[t, a])  (no non-null token: of exp(logp_f[t, a]))
struct VnEvalArgs {
  const float* fclogit;   // (T, n1 + n2) frame heads
  long long ldf;
  int n1, n2, A;
  const int32_t* vids;
  const int32_t* nids;
  const float* attn;      // (nattn, Q): frames (seg_id null) or segment rows
  long long ldattn;
  const int32_t* seg_id;
  int nattn, Q;
  const float* ws;        // (Q, wld): the token stage's rows
  int wld;
  float w1, w;
};

// fl / tk: VL_MAXH floats of LDS each
__device__ inline void vl_eval_frame_row(const VnEvalArgs& e, int t, int32_t* pred, float* fl, float* tk, float* part,
                                         int* parti) {
  const int tid = threadIdx.x;
  const int n1 = e.n1, n2 = e.n2, A = e.A, Q = e.Q, wld = e.wld;
  const int32_t *vids = e.vids, *nids = e.nids;
  const float* ws = e.ws;
  const float w1 = e.w1, w = e.w;
  const int m1 = n1 + 1, m = n1 + n2 + 2;
  float lv, ln;
  vl_stage_row(e.fclogit + (long long)t * e.ldf, n1, n2, fl, part, &lv, &ln);
  const int arow = e.seg_id ? min(max(e.seg_id[t], 0), e.nattn - 1) : t;
  const float* ar = e.attn + (long long)arow * e.ldattn;
  float bv = -INFINITY;
  int bq = 0x7fffffff;
  for (int q = tid; q < Q; q += VL_THREADS) {
    if (ws[(long long)q * wld + m + 1] == 0.f) continue;
    const float x = ar[q];
    if (bq == 0x7fffffff || x > bv) {   // threads visit increasing q: keeps the first max per thread
      bv = x;
      bq = q;
    }
  }
  // a thread's candidate always beats "none"; among candidates the larger value, then the lower token
  float key = bq == 0x7fffffff ? -INFINITY : bv;
  vl_block_argmax(key, bq, part, parti);
  const bool any = bq != 0x7fffffff;
  float zinv_den = 1.f;
  if (any) {
    const float* wr = ws + (long long)bq * wld;
    for (int c = tid; c < m; c += VL_THREADS) tk[c] = wr[c];
    zinv_den = wr[m];
  }
  __syncthreads();
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < A; c += VL_THREADS) {
    const int v = min(max(vids[c], 0), n1 - 1), k = min(max(nids[c], 0), n2 - 1);
    const float lf = fl[v] + fl[n1 + k];
    float p = expf(lf);
    if (any) {
      const float lq = tk[v] + tk[m1 + k];
      p = __fadd_rn(__fmul_rn(w1, expf(lq) / zinv_den), __fmul_rn(w, p));
    }
    if (p > best) {
      best = p;
      bi = c;
    }
  }
  vl_block_argmax(best, bi, part, parti);
  if (tid == 0) pred[t] = bi == 0x7fffffff ? 0 : bi;
}

__global__ __launch_bounds__(VL_THREADS) void vn_eval_frame_kernel(VnEvalArgs e, int32_t* pred) {
  __shared__ float fl[VL_MAXH];
  __shared__ float tk[VL_MAXH];
  __shared__ float part[4];
  __shared__ int parti[4];
  vl_eval_frame_row(e, blockIdx.x, pred, fl, tk, part, parti);
}

// the two stages over every video of a batch: grid (max Q, nvid) / (max T, nvid), a workgroup past its
// video's rows returns at once.  Token rows of video v start at workspace row sum_{u < v} Q_u
__device__ inline long long vl_tok_row0(const fx_vn_video* vv, int vi) {
  long long r = 0;
  for (int u = 0; u < vi; ++u) r += vv[u].Q;
  return r;
}

__global__ __launch_bounds__(VL_THREADS) void vn_eval_tok_batch_kernel(const fx_vn_video* vv, int n1, int n2,
                                                                       const int32_t* vids, const int32_t* nids, int A,
                                                                       float* ws, int wld) {
  __shared__ float sh[VL_MAXH];
  __shared__ float part[4];
  const int vi = blockIdx.y, q = blockIdx.x;
  const fx_vn_video& v = vv[vi];
  if (q >= v.Q) return;
  vl_eval_tok_row(v.action_clogit + (long long)q * v.lda, n1, n2, vids, nids, A,
                  ws + (vl_tok_row0(vv, vi) + q) * wld, sh, part);
}

__global__ __launch_bounds__(VL_THREADS) void vn_eval_frame_batch_kernel(const fx_vn_video* vv, int n1, int n2,
                                                                         const int32_t* vids, const int32_t* nids,
                                                                         int A, const float* ws, int wld, float w1,
                                                                         float w, int32_t* pred) {
  __shared__ float fl[VL_MAXH];
  __shared__ float tk[VL_MAXH];
  __shared__ float part[4];
  __shared__ int parti[4];
  const int vi = blockIdx.y, t = blockIdx.x;
  const fx_vn_video& v = vv[vi];
  if (t >= v.T) return;
  const VnEvalArgs e{v.frame_clogit, v.ldf, n1, n2, A, vids, nids, v.attn, v.ldattn, v.seg_id, v.nattn, v.Q,
                     ws + vl_tok_row0(vv, vi) * wld, wld, w1, w};
  vl_eval_frame_row(e, t, pred + v.pred_off, fl, tk, part, parti);
}

// ---------------------------------------------------------------- matching cost
struct VnMatchArgs {
  const float* aclogit;   // (Q, n1 + n2 + 2) token heads
  long long lda;
  int n1, n2, A;
  const int32_t* vids;
  const int32_t* nids;
  const float* attn;      // (nattn, Q): TDU segment rows (seg_start / seg_end) or frames (seg_start null)
  long long ldattn;
  int nattn;
  const int32_t* seg_start;
  const int32_t* seg_end;
  const int32_t* gs;      // (G) ground-truth segments, inclusive frames, and their actions
  const int32_t* ge;
  const int32_t* gl;
  int G, T;
  float pc, a2fc;
};

// One workgroup per token a.  Pass 1 leaves overlap[a, s] in cost[a, s]: segment-level attention, one
// thread per ground-truth segment walks the TDU segments meeting it in ascending order (found by
// bisection: O(S + G) products per token in all); frame-level attention, one wave per ground-truth
// segment, lanes over its frames, fixed shuffle tree.  col_a = sum_s overlap[a, s] (every thread its
// segments in ascending order, then the fixed tree).  Pass 2: the writer of each entry turns it into the cost.
__device__ inline void vl_match_row(const VnMatchArgs& p, int a, float* crow, float* sh, float* part) {
  const int tid = threadIdx.x;
  const int m1 = p.n1 + 1, m2 = p.n2 + 1;
  float lv, ln;
  vl_stage_row(p.aclogit + (long long)a * p.lda, m1, m2, sh, part, &lv, &ln);
  const float* acol = p.attn + a;
  float colp = 0.f;
  if (p.seg_start) {
    for (int s = tid; s < p.G; s += VL_THREADS) {
      const int g0 = p.gs[s], g1 = p.ge[s];
      int lo = 0, hi = p.nattn;               // first TDU segment ending at or after g0
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.seg_end[mid] < g0) lo = mid + 1;
        else hi = mid;
      }
      float ov = 0.f;
      for (int j = lo; j < p.nattn && p.seg_start[j] <= g1; ++j) {
        const int b0 = max(p.seg_start[j], g0), b1 = min(p.seg_end[j], g1);
        if (b1 >= b0) ov += acol[(long long)j * p.ldattn] * (float)(b1 - b0 + 1);
      }
      crow[s] = ov;
      colp += ov;
    }
  } else {
    const int lane = tid & 63, wv = tid >> 6;
    for (int s = wv; s < p.G; s += VL_THREADS / 64) {
      const int g0 = max(p.gs[s], 0), g1 = min(p.ge[s], p.nattn - 1);
      float ov = 0.f;
      for (int t = g0 + lane; t <= g1; t += 64) ov += acol[(long long)t * p.ldattn];
      ov = vl_wave_sum(ov);
      if (lane == 0) {
        crow[s] = ov;
        colp += ov;
      }
    }
  }
  const float col = vl_block_sum(colp, part);   // (its barriers also publish pass 1's entries to the workgroup)
  for (int s = tid; s < p.G; s += VL_THREADS) {
    const float ov = crow[s];
    const float den = ((float)(p.ge[s] - p.gs[s] + 1) + col) - ov;
    const float iou = den != 0.f ? ov / den : 0.f;
    const int y = min(max(p.gl[s], 0), p.A - 1);
    const int v = min(max(p.vids[y], 0), p.n1 - 1), k = min(max(p.nids[y], 0), p.n2 - 1);
    crow[s] = -p.pc * expf(sh[v] + sh[m1 + k]) - p.a2fc * iou;
  }
}

__global__ __launch_bounds__(VL_THREADS) void vn_match_cost_kernel(VnMatchArgs p, float* cost) {
  __shared__ float sh[VL_MAXH];
  __shared__ float part[4];
  const int a = blockIdx.x;
  vl_match_row(p, a, cost + (long long)a * p.G, sh, part);
}

// every video of a batch: grid (max Q, nvid), cost (nvid, Qmax, Gmax); row (v, a) is the single-video row
// followed by zeros for s >= G_v, a row past its video's tokens all zeros
__global__ __launch_bounds__(VL_THREADS) void vn_match_cost_batch_kernel(const fx_vn_video* vv, int n1, int n2,
                                                                         const int32_t* vids, const int32_t* nids,
                                                                         int A, float pc, float a2fc, int Gmax,
                                                                         float* cost) {
  __shared__ float sh[VL_MAXH];
  __shared__ float part[4];
  const int vi = blockIdx.y, a = blockIdx.x;
  const fx_vn_video& v = vv[vi];
  float* crow = cost + ((long long)vi * gridDim.x + a) * Gmax;
  int G = 0;
  if (a < v.Q) {
    G = v.G;
    const VnMatchArgs p{v.action_clogit, v.lda, n1, n2, A, vids, nids, v.attn, v.ldattn, v.nattn, v.seg_start,
                        v.seg_end, v.gs, v.ge, v.gl, v.G, v.T, pc, a2fc};
    vl_match_row(p, a, crow, sh, part);
  }
  for (int s = G + threadIdx.x; s < Gmax; s += VL_THREADS) crow[s] = 0.f;
}

int vl_check(int n1, int n2, int A, int rows) {
  FX_REQUIRE(n1 > 0 && n2 > 0 && n1 + n2 <= VL_MAXH, "vn_loss: need n1, n2 > 0 and n1 + n2 <= 2048");
  FX_REQUIRE(A > 0 && rows >= 0, "vn_loss: need A > 0 actions and rows >= 0");
  return FX_OK;
}

}  // namespace

// The table's VNCLASS terms (fx_loss_terms_fwd / _bwd, vloss.hip): checks on the host copies before any launch
// (check_vn_terms; a table without such a term, *count == 0, launches nothing of this file), then one
// launch over (FX_LOSS_NB, nterms); workgroups of the other kinds return at once.
static int vn_terms_check(const fx_loss_term& t, bool bwd, long long* lds_floats) {
  const fx_vn_term* m = t.vn_host;
  FX_REQUIRE(m && t.vn, "loss_terms: VNCLASS term without its mapping");
  FX_TRY(vl_check(m->n1, m->n2, m->A, t.R));
  FX_REQUIRE(t.C == m->n1 + m->n2 && t.sc == 1 && t.sr >= t.C, "loss_terms: VNCLASS term needs rows of n1 + n2 logits");
  FX_REQUIRE(m->vids && m->nids, "loss_terms: VNCLASS mapping without id tables");
  FX_REQUIRE(!t.y || t.w, "loss_terms: VNCLASS labels need class weights");
  FX_REQUIRE(!t.rs == !t.re && (!t.rs || (t.y && t.D > 0)),
             "loss_terms: VNCLASS segment targets need frame labels, their count, starts and ends");
  const bool smooth = t.c_sm != 0.f;
  if (bwd) {
    FX_REQUIRE(t.dx && t.dsc == 1 && t.dsr >= t.C, "loss_terms_bwd: VNCLASS term needs a row-major gradient buffer");
    FX_REQUIRE(!smooth || (m->voff && m->vlist && m->noff && m->nlist),
               "loss_terms_bwd: the VNCLASS smooth term needs the CSR lists");
    const long long floats = smooth ? 4LL * t.C + m->A : 2LL * t.C;
    FX_REQUIRE(floats * (long long)sizeof(float) <= VL_MAXLDS,
               "loss_terms_bwd: the VNCLASS smooth term needs 4 (n1 + n2) + A <= 15360 floats of LDS");
    *lds_floats = std::max(*lds_floats, floats);
  }
  return FX_OK;
}

int check_vn_terms(const fx_loss_term* terms_host, int nterms, bool bwd, int* count, long long* lds_floats) {
  *count = 0;
  *lds_floats = 0;
  for (int i = 0; i < nterms; ++i) {
    if (terms_host[i].kind != FX_TERM_VNCLASS) continue;
    FX_TRY(vn_terms_check(terms_host[i], bwd, lds_floats));
    ++*count;
  }
  return FX_OK;
}

void launch_vn_terms_fwd(const fx_loss_term* terms_dev, int nterms, float* part, hipStream_t s) {
  fx_launch(vn_terms_fwd_kernel, dim3(FX_LOSS_NB, nterms), dim3(VL_THREADS), 0, s, terms_dev, part);
}

void launch_vn_terms_bwd(const fx_loss_term* terms_dev, int nterms, const float* gterm, long long lds_floats,
                         hipStream_t s) {
  fx_launch(vn_terms_bwd_kernel, dim3(FX_LOSS_NB, nterms), dim3(VL_THREADS),
            (std::uint32_t)(lds_floats * sizeof(float)), s, terms_dev, gterm);
}

}  // namespace fx

using namespace fx;

extern "C" {

long long fx_vn_workspace_floats(int loss_rows, int tokens, int n1, int n2) {
  return 2LL * std::max(loss_rows, 0) + (long long)std::max(tokens, 0) * (n1 + n2 + 4);
}

int fx_vn_loss_fwd(const float* clogit, long long ld, int R, int n1, int n2, const int32_t* vids, const int32_t* nids,
                   int A, int null, const long long* y, int ny, const int32_t* seg_start, const int32_t* seg_end,
                   const float* w, float c_ce, float c_sm, float* lse, float* out, float* workspace, void* stream) {
  FX_TRY(vl_check(n1, n2, A, R));
  FX_REQUIRE(ld >= n1 + n2, "vn_loss: leading dimension shorter than the row");
  FX_REQUIRE(out && workspace && (R == 0 || (clogit && vids && nids && lse)), "vn_loss: bad arguments");
  FX_REQUIRE(!y || (w && ny > 0), "vn_loss: labels need class weights");
  FX_REQUIRE(!seg_start == !seg_end && (!seg_start || y), "vn_loss: segment mode needs labels, starts and ends");
  FX_REQUIRE(!y || seg_start || ny == R, "vn_loss: hard targets need one label per row");
  hipStream_t s = (hipStream_t)stream;
  VnLossArgs a{clogit, ld, R, n1, n2, A, null ? 1 : 0, vids, nids, y, nullptr, ny, seg_start, seg_end, w, c_sm != 0.f};
  if (R > 0) fx_launch(vn_loss_fwd_kernel, dim3(R), dim3(VL_THREADS), 0, s, a, lse, workspace);
  fx_launch(vn_loss_finish_kernel, dim3(1), dim3(VL_THREADS), 0, s, (const float*)workspace, R, c_ce, c_sm, out);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_vn_loss_bwd(const float* clogit, long long ld, int R, int n1, int n2, const int32_t* vids, const int32_t* nids,
                   int A, int null, const long long* y, int ny, const int32_t* seg_start, const int32_t* seg_end,
                   const float* w, const int32_t* voff, const int32_t* vlist, const int32_t* noff,
                   const int32_t* nlist, const float* lse, float c_ce, float c_sm, const float* gout, float* dclogit,
                   long long lddc, void* stream) {
  FX_TRY(vl_check(n1, n2, A, R));
  FX_REQUIRE(ld >= n1 + n2 && lddc >= n1 + n2, "vn_loss: leading dimension shorter than the row");
  if (R == 0) return FX_OK;
  const int smooth = c_sm != 0.f;
  FX_REQUIRE(clogit && vids && nids && lse && gout && dclogit, "vn_loss_bwd: bad arguments");
  FX_REQUIRE(!y || (w && ny > 0), "vn_loss: labels need class weights");
  FX_REQUIRE(!seg_start == !seg_end && (!seg_start || y), "vn_loss: segment mode needs labels, starts and ends");
  FX_REQUIRE(!y || seg_start || ny == R, "vn_loss: hard targets need one label per row");
  FX_REQUIRE(!smooth || (voff && vlist && noff && nlist), "vn_loss_bwd: the smooth term needs the CSR lists");
  const long long floats = smooth ? 4LL * (n1 + n2) + A : 2LL * (n1 + n2);
  FX_REQUIRE(floats * (long long)sizeof(float) <= VL_MAXLDS,
             "vn_loss_bwd: the smooth term needs 4 (n1 + n2) + A <= 15360 floats of LDS");
  VnLossArgs a{clogit, ld, R, n1, n2, A, null ? 1 : 0, vids, nids, y, nullptr, ny, seg_start, seg_end, w, smooth};
  fx_launch(vn_loss_bwd_kernel, dim3(R), dim3(VL_THREADS), (std::uint32_t)(floats * sizeof(float)),
            (hipStream_t)stream, a, lse, gout, c_ce, c_sm, voff, vlist, noff, nlist, dclogit, lddc);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_vn_eval_pred(const float* action_clogit, long long lda, int Q, const float* frame_clogit, long long ldf, int T,
                    int n1, int n2, const int32_t* vids, const int32_t* nids, int A, const float* attn,
                    long long ldattn, const int32_t* seg_id, int nattn, float mwt, float* workspace, int32_t* pred,
                    void* stream) {
  FX_TRY(vl_check(n1, n2, A, T));
  FX_REQUIRE(n1 + n2 + 2 <= VL_MAXH, "vn_eval_pred: need n1 + n2 + 2 <= 2048 token head columns");
  FX_REQUIRE(Q > 0 && lda >= n1 + n2 + 2 && ldf >= n1 + n2 && ldattn >= Q, "vn_eval_pred: bad sizes");
  FX_REQUIRE(seg_id ? nattn > 0 : nattn == T, "vn_eval_pred: frame-level attention needs one row per frame");
  if (T == 0) return FX_OK;
  FX_REQUIRE(action_clogit && frame_clogit && vids && nids && attn && workspace && pred, "vn_eval_pred: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int wld = n1 + n2 + 4;
  fx_launch(vn_eval_tok_kernel, dim3(Q), dim3(VL_THREADS), 0, s, action_clogit, lda, n1, n2, vids, nids, A, workspace,
            wld);
  const float w1 = (float)(1.0 - (double)mwt);
  const VnEvalArgs e{frame_clogit, ldf, n1, n2, A, vids, nids, attn, ldattn, seg_id, nattn, Q, workspace, wld, w1, mwt};
  fx_launch(vn_eval_frame_kernel, dim3(T), dim3(VL_THREADS), 0, s, e, pred);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_vn_match_cost(const float* action_clogit, long long lda, int Q, int n1, int n2, const int32_t* vids,
                     const int32_t* nids, int A, const float* attn, long long ldattn, int nattn,
                     const int32_t* seg_start, const int32_t* seg_end, const int32_t* gs, const int32_t* ge,
                     const int32_t* gl, int G, int T, float pc, float a2fc, float* cost, void* stream) {
  FX_TRY(vl_check(n1, n2, A, Q));
  FX_REQUIRE(n1 + n2 + 2 <= VL_MAXH, "vn_match_cost: need n1 + n2 + 2 <= 2048 token head columns");
  FX_REQUIRE(G > 0 && T > 0 && nattn > 0, "vn_match_cost: need ground-truth segments, frames and attention rows");
  FX_REQUIRE(lda >= n1 + n2 + 2 && ldattn >= Q, "vn_match_cost: leading dimension shorter than the row");
  FX_REQUIRE(!seg_start == !seg_end, "vn_match_cost: segment-level attention needs starts and ends");
  FX_REQUIRE(seg_start ? nattn <= T : nattn == T,
             "vn_match_cost: frame-level attention needs one row per frame, segment-level at most T rows");
  if (Q == 0) return FX_OK;
  FX_REQUIRE(action_clogit && vids && nids && attn && gs && ge && gl && cost, "vn_match_cost: bad arguments");
  VnMatchArgs p{action_clogit, lda, n1, n2, A, vids, nids, attn, ldattn, nattn, seg_start, seg_end, gs, ge, gl, G, T,
                pc, a2fc};
  fx_launch(vn_match_cost_kernel, dim3(Q), dim3(VL_THREADS), 0, (hipStream_t)stream, p, cost);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_vn_match_cost_batch(const fx_vn_video* vids_host, const fx_vn_video* vids_dev, int nvid, int n1, int n2,
                           const int32_t* vids, const int32_t* nids, int A, float pc, float a2fc, int Gmax,
                           float* cost, void* stream) {
  FX_REQUIRE(nvid >= 0 && (nvid == 0 || (vids_host && vids_dev)), "vn_match_cost_batch: bad arguments");
  FX_TRY(vl_check(n1, n2, A, 0));
  FX_REQUIRE(n1 + n2 + 2 <= VL_MAXH, "vn_match_cost_batch: need n1 + n2 + 2 <= 2048 token head columns");
  int Qmax = 0;
  for (int i = 0; i < nvid; ++i) {
    const fx_vn_video& v = vids_host[i];
    FX_REQUIRE(v.Q >= 0 && v.G > 0 && v.T > 0 && v.nattn > 0,
               "vn_match_cost_batch: need ground-truth segments, frames and attention rows");
    FX_REQUIRE(v.G <= Gmax, "vn_match_cost_batch: a video has more ground-truth segments than Gmax");
    FX_REQUIRE(v.lda >= n1 + n2 + 2 && v.ldattn >= v.Q, "vn_match_cost_batch: leading dimension shorter than the row");
    FX_REQUIRE(!v.seg_start == !v.seg_end, "vn_match_cost_batch: segment-level attention needs starts and ends");
    FX_REQUIRE(v.seg_start ? v.nattn <= v.T : v.nattn == v.T,
               "vn_match_cost_batch: frame-level attention needs one row per frame, segment-level at most T rows");
    FX_REQUIRE(v.Q == 0 || (v.action_clogit && v.attn && v.gs && v.ge && v.gl), "vn_match_cost_batch: bad arguments");
    Qmax = std::max(Qmax, v.Q);
  }
  if (Qmax == 0) return FX_OK;
  FX_REQUIRE(vids && nids && cost && nvid <= 65535, "vn_match_cost_batch: bad arguments");
  fx_launch(vn_match_cost_batch_kernel, dim3(Qmax, nvid), dim3(VL_THREADS), 0, (hipStream_t)stream, vids_dev, n1, n2,
            vids, nids, A, pc, a2fc, Gmax, cost);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_vn_eval_pred_batch(const fx_vn_video* vids_host, const fx_vn_video* vids_dev, int nvid, int n1, int n2,
                          const int32_t* vids, const int32_t* nids, int A, float mwt, float* workspace, int32_t* pred,
                          void* stream) {
  FX_REQUIRE(nvid >= 0 && (nvid == 0 || (vids_host && vids_dev)), "vn_eval_pred_batch: bad arguments");
  FX_TRY(vl_check(n1, n2, A, 0));
  FX_REQUIRE(n1 + n2 + 2 <= VL_MAXH, "vn_eval_pred_batch: need n1 + n2 + 2 <= 2048 token head columns");
  int Qmax = 0, Tmax = 0;
  for (int i = 0; i < nvid; ++i) {
    const fx_vn_video& v = vids_host[i];
    FX_REQUIRE(v.T >= 0 && v.Q > 0 && v.lda >= n1 + n2 + 2 && v.ldf >= n1 + n2 && v.ldattn >= v.Q && v.pred_off >= 0,
               "vn_eval_pred_batch: bad sizes");
    FX_REQUIRE(v.seg_id ? v.nattn > 0 : v.nattn == v.T,
               "vn_eval_pred_batch: frame-level attention needs one row per frame");
    FX_REQUIRE(v.T == 0 || (v.action_clogit && v.frame_clogit && v.attn), "vn_eval_pred_batch: bad arguments");
    if (v.T > 0) Qmax = std::max(Qmax, v.Q);
    Tmax = std::max(Tmax, v.T);
  }
  if (Tmax == 0) return FX_OK;
  FX_REQUIRE(vids && nids && workspace && pred && nvid <= 65535, "vn_eval_pred_batch: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int wld = n1 + n2 + 4;
  fx_launch(vn_eval_tok_batch_kernel, dim3(Qmax, nvid), dim3(VL_THREADS), 0, s, vids_dev, n1, n2, vids, nids, A,
            workspace, wld);
  const float w1 = (float)(1.0 - (double)mwt);
  fx_launch(vn_eval_frame_batch_kernel, dim3(Tmax, nvid), dim3(VL_THREADS), 0, s, vids_dev, n1, n2, vids, nids, A,
            (const float*)workspace, wld, w1, mwt, pred);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // extern "C"
