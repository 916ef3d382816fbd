// Attention entry points: the multi-head core as batched GEMMs + row softmax, and the fused attention of
// queries over T frames -- its launch plan (tattn_plan), the one function that issues a plan's launches
// and the two launchers of ops.h; the kernels are attn_t_lds.hip and attn_t_rr.hip.
#include <algorithm>
#include <cmath>

#include "attn_t_dev.h"
#include "fx_common.h"
#include "ops.h"

using namespace fx;

// ---------------------------------------------------------------- attention over T: plan and launches
namespace fx {
using namespace attn_t_dev;
namespace {

enum class TAttnFamily { LDS, RR };                    // attn_t_lds.hip / attn_t_rr.hip
enum class TAttnMerge { NONE, IN_LAUNCH, LAUNCH };     // one chunk / fold_merge / tattn_merge_kernel
struct TAttnPlan {
  TAttnFamily family;
  int Tc, KT, nsplit;     // keys per chunk (register-resident: 128 KT), chunks of the longest video
  int Qp, Hp;             // partial tile: padded queries of a block, padded head dim
  int nqb;                // query blocks of QB, one launch (and merge launch) each
  size_t lds, merge_lds;  // dynamic LDS bytes of the kernel and of the merge launch
  TAttnMerge merge;
  long long ws_floats;    // partial workspace of one query block (TAttnWs)
};

// Every launch decision of a call, from its sizes alone (no HIP call, no knob).  Tmax: the longest
// video's key count; aligned: 16-B loads of every row slice (TAttnArgs::vec).
//   family: register-resident for head dim 32, <= 32 queries and aligned rows -- 32 KT keys per wave, KT = 2
//     (256-key chunks) unless that leaves fewer than one workgroup per CU, then KT = 1;
//   LDS-staged chunk: the largest power of two in [32, 256] whose LDS images fit (Tc * Hp <= NVK float4 per
//     thread; forward: at most 8 score tiles, two per wave, in registers), halved while the launch has fewer
//     than ~256 workgroups (smaller chunks at full occupancy measured slower: round 4);
//   merge: inside the launch for the register-resident family with <= FOLD_MAX chunks and a counter per
//     (video, head) -- tattn_run falls back to the merge launch when the stream has no counters.
TAttnPlan tattn_plan(int nvid, int Qv, int Tmax, int hd, int nh, bool bwd, bool aligned) {
  constexpr int kMinWorkgroups = 256;   // one per CU
  auto chunks = [&](int Tc) { return (Tmax + Tc - 1) / Tc; };
  TAttnPlan p{};
  p.nqb = (Qv + QB - 1) / QB;
  if (hd == 32 && Qv <= 32 && aligned) {
    p.family = TAttnFamily::RR;
    p.KT = (long long)nvid * nh * chunks(256) >= kMinWorkgroups ? 2 : 1;
    p.Tc = 128 * p.KT;
    p.Qp = p.Hp = 32;
  } else {
    p.family = TAttnFamily::LDS;
    p.Qp = std::max(32, (std::min(Qv, QB) + 31) / 32 * 32);
    p.Hp = std::max(32, (hd + 31) / 32 * 32);
    auto lds_b = [&](int Tc) {
      const size_t q = bwd ? 2 : 1, pp = bwd ? 2 : 1;
      return sizeof(float) * (q * p.Qp * (p.Hp + 4) + 2 * (size_t)Tc * (p.Hp + 4) + pp * p.Qp * (Tc + 4) + 4 * 1024 +
                              2 * p.Qp + 4);
    };
    int Tc = 256;
    while (Tc > 32 && (lds_b(Tc) > 150 * 1024 || Tc * p.Hp > NVK * 4 * AT || Tc * p.Qp > 8 * 1024)) Tc >>= 1;
    while (Tc > 32 && (long long)nvid * nh * chunks(Tc) < kMinWorkgroups) Tc >>= 1;
    p.Tc = Tc;
    p.lds = lds_b(Tc);
  }
  p.nsplit = std::max(1, chunks(p.Tc));
  p.merge = p.nsplit == 1 ? TAttnMerge::NONE
            : p.family == TAttnFamily::RR && p.nsplit <= FOLD_MAX && (long long)nvid * nh <= kArrivalCounters
                ? TAttnMerge::IN_LAUNCH
                : TAttnMerge::LAUNCH;
  // the forward merge keeps the chunks' (m, l) rows in LDS; the backward merge only adds tiles
  p.merge_lds = bwd ? 0 : sizeof(float) * 2 * (size_t)p.nsplit * p.Qp;
  // (the LDS-staged launches have always asked for the merge's bytes as well: part of their occupancy)
  if (p.family == TAttnFamily::LDS) p.lds = std::max(p.lds, sizeof(float) * 2 * (size_t)p.nsplit * p.Qp + 16);
  p.ws_floats = TAttnWs(nvid, nh, p.nsplit, p.Qp, p.Hp).floats();
  return p;
}

bool a16(const void* p, long long ld) { return p == nullptr || (((uintptr_t)p & 15) == 0 && (ld & 3) == 0); }

// shared argument set-up: key offsets (uniform Tv per video when opt->koff is NULL), dropout
int tattn_setup(TAttnArgs& a, int nvid, int Qv, int Tv, int hd, int nh, const TAttnOpts* opt, int& Tmax) {
  FX_REQUIRE(nvid >= 1 && nvid <= MAXV && Qv >= 1 && hd >= 1 && hd <= 64 && nh >= 1,
             "attention over T: 1..32 videos, >= 1 query, head dim <= 64");
  Tmax = 0;
  a.koff[0] = 0;
  for (int v = 0; v < nvid; ++v) {
    const int k0 = opt && opt->koff ? opt->koff[v] : v * Tv, k1 = opt && opt->koff ? opt->koff[v + 1] : (v + 1) * Tv;
    FX_REQUIRE(k1 > k0 && k0 >= 0, "attention over T: every video needs >= 1 key row, offsets increasing");
    a.koff[v] = k0;
    a.koff[v + 1] = k1;
    Tmax = std::max(Tmax, k1 - k0);
  }
  a.ktot = a.koff[nvid];
  int Qmax = 0;
  for (int v = 0; v <= nvid; ++v) {
    a.qoff[v] = opt && opt->qoff ? opt->qoff[v] : v * Qv;
    if (v > 0) {
      FX_REQUIRE(a.qoff[v] > a.qoff[v - 1], "attention over T: every video needs >= 1 query row, offsets increasing");
      Qmax = std::max(Qmax, a.qoff[v] - a.qoff[v - 1]);
    }
  }
  FX_REQUIRE(a.qoff[0] >= 0 && Qmax <= Qv, "attention over T: query offsets from >= 0, Qv the longest video");
  const float p = opt ? opt->drop_p : 0.f;
  FX_REQUIRE(p >= 0.f && p < 1.f, "attention over T: dropout p in [0, 1)");
  a.drop_p = p;
  a.drop_thr = p > 0.f ? std::max(fx_drop_thresh(p), 1u) : 0u;
  a.drop_seed = opt ? opt->drop_seed : 0ull;
  a.hd = hd;
  a.nh = nh;
  a.qs = Qv;
  return FX_OK;
}

// The launches of plan p for the filled arguments a, either direction: per query block of QB the family's
// kernel and, unless one chunk or the in-launch merge covers it, the merge launch.  Backward: a later
// block ADDS its dK / dV to the earlier blocks' (same key rows).  Opens the direction's profiling bracket
// once the plan is known to be launchable; the caller closes it with the direction's flops and bytes.
int tattn_run(const TAttnPlan& p, TAttnArgs& a, int nvid, int Qv, bool bwd, bool acc_kv, hipStream_t s) {
  FX_REQUIRE(a.ws || p.nsplit == 1, "attention over T: workspace required");
  FX_REQUIRE(p.lds <= 160 * 1024, "attention over T: LDS images too large");
  FX_REQUIRE(p.merge_lds <= 160 * 1024, "attention over T: too many frames per video for the in-LDS merge");
  a.Qp = p.Qp; a.Hp = p.Hp; a.Tc = p.Tc; a.nsplit = p.nsplit;
  // (a stream without arrival counters: null, and the partials go to the merge launch instead)
  a.cnt = p.merge == TAttnMerge::IN_LAUNCH ? arrival_counters(s) : nullptr;
  prof_begin(bwd ? 2 : 1, s);
  const dim3 grid(p.nsplit, a.nh, nvid);
  for (int q0 = 0; q0 < Qv; q0 += QB) {
    a.q0 = q0;
    a.Qv = std::min(QB, Qv - q0);
    a.acc_kv = bwd && (q0 > 0 || acc_kv);
    if (p.family == TAttnFamily::RR) launch_tattn_rr(a, bwd, p.KT, grid, s);
    else launch_tattn_lds(a, bwd, grid, p.lds, s);
    FX_CHECK_HIP(hipGetLastError());
    if (p.nsplit > 1 && !a.cnt) {
      launch_tattn_merge(a, nvid, !bwd, bwd ? a.scale : 1.f, p.merge_lds, s);
      FX_CHECK_HIP(hipGetLastError());
    }
  }
  return FX_OK;
}

}  // namespace

// the largest partial workspace a call of these sizes can be planned with: either direction, rows aligned or not
long long tattn_ws_floats(int nvid, int Qv, int Tv, int hd, int nh) {
  long long w = 0;
  for (int i = 0; i < 4; ++i) w = std::max(w, tattn_plan(nvid, Qv, Tv, hd, nh, i & 1, i & 2).ws_floats);
  return w;
}

int launch_tattn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                     int nvid, int Qv, int Tv, int hd, int nh, float scale, float* o, long long ldo, float* lse,
                     float* ws, hipStream_t s, const TAttnOpts* opt) {
  TAttnArgs a{};
  int Tmax = 0;
  FX_TRY(tattn_setup(a, nvid, Qv, Tv, hd, nh, opt, Tmax));
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv;
  a.out = o; a.ld_out = ldo; a.lse = lse; a.ws = ws;
  a.scale = scale;
  a.vec = (hd % 4 == 0) && a16(q, ldq) && a16(k, ldk) && a16(v, ldv);
  const TAttnPlan p = tattn_plan(nvid, Qv, Tmax, hd, nh, false, a.vec);
  FX_TRY(tattn_run(p, a, nvid, Qv, false, false, s));
  // algorithmic traffic: K and V rows read once per query block, q read, o and lse written
  const double kv = (double)a.ktot * nh * hd * p.nqb, qo = (double)nvid * Qv * nh * hd;
  prof_end(1, s, 4.0 * qo * (double)a.ktot / nvid, 4.0 * (2.0 * kv + 2.0 * qo + (double)nvid * nh * Qv));
  return FX_OK;
}

int launch_tattn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                     const float* o, long long ldo, const float* dout, long long lddo, const float* lse, int nvid,
                     int Qv, int Tv, int hd, int nh, float scale, float* dq, long long lddq, float* dk, long long lddk,
                     float* dv, long long lddv, float* ws, hipStream_t s, const TAttnOpts* opt) {
  TAttnArgs a{};
  int Tmax = 0;
  FX_TRY(tattn_setup(a, nvid, Qv, Tv, hd, nh, opt, Tmax));
  FX_REQUIRE(dq && dk && dv, "attention over T backward: dq, dk, dv required");
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv;
  a.o = o; a.ldo = ldo; a.dout = dout; a.lddo = lddo;
  a.out = dq; a.ld_out = lddq; a.dk = dk; a.lddk = lddk; a.dv = dv; a.lddv = lddv;
  a.lse = const_cast<float*>(lse); a.ws = ws;
  a.scale = scale;
  a.vec = (hd % 4 == 0) && a16(q, ldq) && a16(k, ldk) && a16(v, ldv) && a16(o, ldo) && a16(dout, lddo);
  const TAttnPlan p = tattn_plan(nvid, Qv, Tmax, hd, nh, true, a.vec);
  FX_TRY(tattn_run(p, a, nvid, Qv, true, opt && opt->acc_kv, s));
  // algorithmic traffic: K, V read and dK, dV written once per query block; q, o, dout, lse read, dq written.
  // flops: S = qK^T recomputed, dP = dO V^T, dV = P^T dO, dK = dS^T q, dq = dS K
  const double kv = (double)a.ktot * nh * hd * p.nqb, qo = (double)nvid * Qv * nh * hd;
  prof_end(2, s, 10.0 * qo * (double)a.ktot / nvid, 4.0 * (4.0 * kv + 4.0 * qo + (double)nvid * nh * Qv));
  return FX_OK;
}

}  // namespace fx

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
