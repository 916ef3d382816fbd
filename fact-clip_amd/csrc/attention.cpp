// Attention entry points: the multi-head core as batched GEMMs + row softmax, and the fused attention of
// queries over T frames (attn_t.hip).
#include <algorithm>
#include <cmath>

#include "fx_common.h"
#include "ops.h"

using namespace fx;

extern "C" {

// ---------------------------------------------------------------- MHA core
long long fx_mha_core_workspace_floats(int Lq, int Lk, int E, int nhead) {
  const int hd = E / std::max(nhead, 1);
  long long ws = 2LL * nhead * Lq * Lk;   // dropped probabilities, dS
  long long sp = 0;
  sp = std::max(sp, split_ws(Lq, hd, Lk, nhead));
  sp = std::max(sp, split_ws(Lk, hd, Lq, nhead));
  sp = std::max(sp, split_ws(Lq, Lk, hd, nhead));
  return ws + 2 * sp;
}

int fx_mha_core_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                    int Lq, int Lk, int E, int nhead, float drop_p, unsigned long long seed, float* probs, float* o,
                    long long ldo, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(nhead > 0 && E % nhead == 0, "mha: E must be divisible by nhead");
  FX_REQUIRE(drop_p == 0.f || workspace, "mha: dropout needs the workspace");
  const int hd = E / nhead;
  const float scale = 1.0f / std::sqrt((float)hd);
  const long long nLL = (long long)nhead * Lq * Lk;
  float* spl = workspace ? workspace + 2 * nLL : nullptr;
  WsBound wb(spl, workspace ? fx_mha_core_workspace_floats(Lq, Lk, E, nhead) - 2 * nLL : 0);
  // S_h = (Q_h K_h^T) * scale  -> probs buffer, then row softmax in place
  fx_gemm_desc d = gemm_desc(Lq, Lk, hd, op_rows(q, ldq), op_rows(k, ldk), probs, Lk);
  d.batch = nhead;
  d.a.batch_stride = hd;
  d.b.batch_stride = hd;
  d.c_batch_stride = (long long)Lq * Lk;
  d.alpha = scale;
  FX_TRY(launch_gemm(d, s));
  FX_TRY(launch_softmax_rows(probs, Lk, nhead * Lq, Lk, 1.f, probs, Lk, s));
  // attention dropout (nn.MultiheadAttention dropout=attn_dropout): O = dropout(P) V, mask index
  // (h Lq + i) Lk + j
  const float* pv = probs;
  if (drop_p > 0.f) {
    FX_TRY(launch_dropout(probs, Lk, nhead * Lq, Lk, Lk, 0, drop_p, seed, workspace, Lk, s));
    pv = workspace;
  }
  // O_h = P_h V_h
  fx_gemm_desc e = gemm_desc(Lq, hd, Lk, op_rows(pv, Lk), op_cols(v, ldv), o, ldo);
  e.batch = nhead;
  e.a.batch_stride = (long long)Lq * Lk;
  e.b.batch_stride = hd;
  e.c_batch_stride = hd;
  e.split_k = workspace ? pick_split(Lq, hd, Lk, nhead) : 1;
  e.workspace = spl;
  return launch_gemm(e, s);
}

int fx_mha_core_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                    const float* probs, const float* dout, long long lddo, int Lq, int Lk, int E, int nhead,
                    float drop_p, unsigned long long seed, float* dq, long long lddq, float* dk, long long lddk,
                    float* dv, long long lddv, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(nhead > 0 && E % nhead == 0, "mha: E must be divisible by nhead");
  const int hd = E / nhead;
  const float scale = 1.0f / std::sqrt((float)hd);
  const long long nLL = (long long)nhead * Lq * Lk;
  float* pd = workspace;
  float* dS = workspace + nLL;
  float* spl = workspace + 2 * nLL;
  WsBound wb(spl, fx_mha_core_workspace_floats(Lq, Lk, E, nhead) - 2 * nLL);
  // dP_h = dO_h V_h^T   (through the dropout: the same mask and scale)
  fx_gemm_desc d = gemm_desc(Lq, Lk, hd, op_rows(dout, lddo), op_rows(v, ldv), dS, Lk);
  d.batch = nhead;
  d.a.batch_stride = hd;
  d.b.batch_stride = hd;
  d.c_batch_stride = (long long)Lq * Lk;
  FX_TRY(launch_gemm(d, s));
  const float* pv = probs;
  if (drop_p > 0.f) {
    FX_TRY(launch_dropout(dS, Lk, nhead * Lq, Lk, Lk, 0, drop_p, seed, dS, Lk, s));
    FX_TRY(launch_dropout(probs, Lk, nhead * Lq, Lk, Lk, 0, drop_p, seed, pd, Lk, s));
    pv = pd;
  }
  // dS = softmax_bwd(P, dP)
  FX_TRY(launch_softmax_rows_bwd(probs, Lk, dS, Lk, nullptr, 0, nhead * Lq, Lk, 1.f, dS, Lk, s));
  // dQ_h = scale * dS_h K_h
  if (dq) {
    fx_gemm_desc e = gemm_desc(Lq, hd, Lk, op_rows(dS, Lk), op_cols(k, ldk), dq, lddq);
    e.batch = nhead;
    e.a.batch_stride = (long long)Lq * Lk;
    e.b.batch_stride = hd;
    e.c_batch_stride = hd;
    e.alpha = scale;
    e.split_k = pick_split(Lq, hd, Lk, nhead);
    e.workspace = spl;
    FX_TRY(launch_gemm(e, s));
  }
  // dK_h = scale * dS_h^T Q_h
  if (dk) {
    fx_gemm_desc e = gemm_desc(Lk, hd, Lq, op_cols(dS, Lk), op_cols(q, ldq), dk, lddk);
    e.batch = nhead;
    e.a.batch_stride = (long long)Lq * Lk;
    e.b.batch_stride = hd;
    e.c_batch_stride = hd;
    e.alpha = scale;
    e.split_k = pick_split(Lk, hd, Lq, nhead);
    e.workspace = spl;
    FX_TRY(launch_gemm(e, s));
  }
  // dV_h = dropout(P_h)^T dO_h
  if (dv) {
    fx_gemm_desc e = gemm_desc(Lk, hd, Lq, op_cols(pv, Lk), op_cols(dout, lddo), dv, lddv);
    e.batch = nhead;
    e.a.batch_stride = (long long)Lq * Lk;
    e.b.batch_stride = hd;
    e.c_batch_stride = hd;
    e.split_k = pick_split(Lk, hd, Lq, nhead);
    e.workspace = spl;
    FX_TRY(launch_gemm(e, s));
  }
  return FX_OK;
}

// ---------------------------------------------------------------- MHA over T (fused)
long long fx_mha_t_workspace_floats(int nvid, int Lq, int T, int hd, int nhead) {
  return tattn_ws_floats(nvid, Lq, T, hd, nhead);
}

int fx_mha_t_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, int nvid,
                 int Lq, int T, int hd, int nhead, float scale, float* o, long long ldo, float* lse, float* workspace,
                 void* stream) {
  return launch_tattn_fwd(q, ldq, k, ldk, v, ldv, nvid, Lq, T, hd, nhead, scale, o, ldo, lse, workspace,
                          (hipStream_t)stream);
}

int fx_mha_t_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                 const float* o, long long ldo, const float* dout, long long lddo, const float* lse, int nvid, int Lq,
                 int T, int hd, int nhead, float scale, float* dq, long long lddq, float* dk, long long lddk, float* dv,
                 long long lddv, float* workspace, void* stream) {
  return launch_tattn_bwd(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, nvid, Lq, T, hd, nhead, scale, dq, lddq, dk,
                          lddk, dv, lddv, workspace, (hipStream_t)stream);
}

}  // extern "C"
