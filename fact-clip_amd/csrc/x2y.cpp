// X2Y_map: single-head cross attention between frame rows and token rows, forward and backward.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fx_common.h"
#include "ops.h"

using namespace fx;

// Single-head cross attention of basic.py:349-389 (kq_pos=True), nvid videos stacked by rows:
// video v owns X rows [x_off[v], x_off[v+1]) and Y rows [y_off[v], y_off[v+1]) (host prefix arrays,
// NULL for one video); projections run over all rows at once, the attention core per video.
// logit / attn hold each video's (ny_v x nx_v) block, packed in video order.
// saved: xin (Nx*xdim, X+Xpos when Xpos), yin (Ny*ydim), xk, xv (Nx*Hd), yq, feat (Ny*Hd)
namespace {
constexpr int GMAX_GROUP = 4;   // members of one grouped direct-GEMM launch (gemm_dev.h GMAX)
struct X2YLayout {
  long long xin, yin, xk, xv, yq, feat, total;
};
X2YLayout x2y_layout(int Nx, int xdim, int Ny, int ydim, int Hd) {
  X2YLayout L{};
  L.xin = 0;
  L.yin = L.xin + al64((long long)Nx * xdim);
  L.xk = L.yin + al64((long long)Ny * ydim);
  L.xv = L.xk + al64((long long)Nx * Hd);
  L.yq = L.xv + al64((long long)Nx * Hd);
  L.feat = L.yq + al64((long long)Ny * Hd);
  L.total = L.feat + al64((long long)Ny * Hd);
  return L;
}
struct VidRows {
  int n;
  std::vector<int> x, y;        // prefix offsets (n + 1)
  std::vector<long long> a;     // attention block offsets (n + 1)
};
VidRows vid_rows(int Nx, int Ny, int nvid, const int* x_off, const int* y_off) {
  VidRows v;
  v.n = std::max(nvid, 1);
  if (v.n == 1 || !x_off || !y_off) {
    v.n = 1;
    v.x = {0, Nx};
    v.y = {0, Ny};
  } else {
    v.x.assign(x_off, x_off + v.n + 1);
    v.y.assign(y_off, y_off + v.n + 1);
  }
  v.a.assign(v.n + 1, 0);
  for (int i = 0; i < v.n; ++i)
    v.a[i + 1] = v.a[i] + (long long)(v.y[i + 1] - v.y[i]) * (v.x[i + 1] - v.x[i]);
  return v;
}
long long x2y_split_ws1(int Nx, int xdim, int Ny, int ydim, int Hd, int outdim) {
  long long sp = 0;
  sp = std::max(sp, split_ws(Ny, Nx, Hd));             // logits
  sp = std::max(sp, split_ws(Ny, Hd, Nx));             // feat, dyq
  sp = std::max(sp, split_ws(Nx, Hd, Ny));             // dxv, dxk
  sp = std::max(sp, split_ws(Ny, ydim + Hd, outdim));  // dcat
  sp = std::max(sp, dwdb_ws(Ny, ydim, outdim));        // dW_y pieces (+ bias column)
  sp = std::max(sp, dwdb_ws(Ny, Hd, outdim));
  sp = std::max(sp, dwdb_ws(Nx, xdim, Hd));            // dW_k / dW_v
  sp = std::max(sp, dwdb_ws(Ny, ydim, Hd));            // dW_q
  sp = std::max(sp, split_ws(Nx, xdim, Hd));           // dX
  sp = std::max(sp, split_ws(Ny, ydim, Hd));           // dY
  return sp;
}
long long x2y_split_ws(const VidRows& v, int xdim, int ydim, int Hd, int outdim) {
  long long sp = x2y_split_ws1(v.x[v.n], xdim, v.y[v.n], ydim, Hd, outdim);
  if (Hd % 32 == 0) sp = std::max(sp, x2y_a2f_dw_ws_floats(v.n, Hd, v.x.data()));   // (the a2f dW kernel's partials)
  for (int i = 0; i < v.n; ++i)
    sp = std::max(sp, x2y_split_ws1(v.x[i + 1] - v.x[i], xdim, v.y[i + 1] - v.y[i], ydim, Hd, outdim));
  return sp;
}
// split-K slabs of the weight-gradient GEMMs on the side stream (their own region: the main stream's
// GEMMs keep using the x2y split region meanwhile)
long long x2y_side_ws(int Nx, int xdim, int Ny, int ydim, int Hd, int outdim) {
  auto one = [](int rows, int M, int N) {
    const int sp = std::max(pick_split(M, N, rows), defer_split(rows));
    return sp > 1 ? (long long)sp * M * N : 0LL;
  };
  // without dropout dW_y is two GEMMs ([Y | 1] and feat), each narrower than the concatenation and so
  // possibly split more ways (fewer tiles): a 1724-row ragged batch split the [Y | 1] piece 7 ways
  // where the concatenation takes 3
  long long w = std::max(one(Ny, outdim, ydim + Hd + 1), one(Nx, Hd, xdim + 1));
  w = std::max(w, std::max(one(Ny, outdim, ydim + 1), one(Ny, outdim, Hd + 1)));
  return std::max(w, one(Ny, Hd, ydim + 1));
}
// workspace (float offsets; every region up to `side` starts 64-float aligned):
// [dcat][dL][dxv][dxk][dyq][dXk][dYq] the backward's intermediates, [split] split-K slabs of the main
// stream's GEMMs (the forward's sit at offset 0, over the intermediates it does not use), [colsum],
// [catd] the dropped cat[Y, feat] (dropout only), [side] slabs of the side stream's weight-gradient GEMMs,
// [f2a] the fused f2a cores' per-chunk partials
struct X2YWs {
  long long dcat, dL, dxv, dxk, dyq, dXk, dYq, split, split_floats, colsum, catd, side, side_floats, f2a, total;
};
X2YWs x2y_ws_layout(int Nx, int xdim, int Ny, int ydim, int Hd, int outdim, const VidRows& v) {
  X2YWs W{};
  W.dcat = 0;
  W.dL = W.dcat + al64((long long)Ny * (ydim + Hd));
  W.dxv = W.dL + al64(v.a[v.n]);
  W.dxk = W.dxv + al64((long long)Nx * Hd);
  W.dyq = W.dxk + al64((long long)Nx * Hd);
  W.dXk = W.dyq + al64((long long)Ny * Hd);
  W.dYq = W.dXk + al64((long long)Nx * xdim);
  W.split = W.dYq + al64((long long)Ny * ydim);
  W.split_floats = x2y_split_ws(v, xdim, ydim, Hd, outdim);
  W.colsum = W.split + al64(W.split_floats);
  W.catd = W.colsum + al64(colsum_workspace_floats(std::max(Nx, Ny), std::max(Hd, outdim)));
  W.side = W.catd + al64((long long)Ny * (ydim + Hd));
  W.side_floats = x2y_side_ws(Nx, xdim, Ny, ydim, Hd, outdim);
  W.f2a = W.side + W.side_floats;
  W.total = W.f2a + x2y_f2a_ws_floats(v.n, v.x.data(), v.y.data(), Hd);
  return W;
}
}  // namespace
extern "C" {

long long fx_x2y_saved_floats(int Nx, int xdim, int Ny, int ydim, int Hd) {
  return x2y_layout(Nx, xdim, Ny, ydim, Hd).total;
}

long long fx_x2y_workspace_floats(int Nx, int xdim, int Ny, int ydim, int Hd, int outdim, int nvid,
                                  const int* x_off, const int* y_off) {
  return x2y_ws_layout(Nx, xdim, Ny, ydim, Hd, outdim, vid_rows(Nx, Ny, nvid, x_off, y_off)).total;
}

int fx_x2y_core(int Hd, int nvid, const int* x_off, const int* y_off, int Nx, int Ny) {
  if (Hd <= 0 || Nx < 0 || Ny < 0) return 0;
  const VidRows v = vid_rows(Nx, Ny, nvid, x_off, y_off);
  switch (x2y_core_pick(v.n, v.x.data(), v.y.data(), Hd)) {
    case FX_X2Y_CORE_A2F:
    case FX_X2Y_CORE_A2F_WIDE: return 1;
    case FX_X2Y_CORE_F2A:
    case FX_X2Y_CORE_F2A_WIDE: return 2;
    default: return 0;
  }
}

// catd = dropout(cat[Y, feat]) (basic.py:382), mask index r (ydim + Hd) + c
static int x2y_drop_cat(const float* Y, long long ldy, const float* feat, int Ny, int ydim, int Hd, float p,
                        unsigned long long seed, float* catd, hipStream_t s) {
  const int cw = ydim + Hd;
  FX_TRY(launch_dropout(Y, ldy, Ny, ydim, cw, 0, p, seed, catd, cw, s));
  return launch_dropout(feat, Hd, Ny, Hd, cw, ydim, p, seed, catd + ydim, cw, s);
}

int fx_x2y_fwd(const float* X, long long ldx, int Nx, int xdim, const float* Xpos, long long ldxp, int xpos_cols,
               const float* Y, long long ldy, int Ny, int ydim, const float* Ypos, long long ldyp, int ypos_cols,
               const float* wk, const float* bk, const float* wv, const float* bv, const float* wq, const float* bq,
               const float* wy, const float* by, int Hd, int outdim, int nvid, const int* x_off, const int* y_off,
               float drop_p, unsigned long long seed, float* out, long long ldo, float* logit, float* attn,
               float* saved, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const VidRows V = vid_rows(Nx, Ny, nvid, x_off, y_off);
  FX_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "x2y: dropout must be in [0, 1)");
  FX_REQUIRE(V.x[V.n] == Nx && V.y[V.n] == Ny, "x2y: offsets must end at Nx / Ny");
  const X2YLayout L = x2y_layout(Nx, xdim, Ny, ydim, Hd);
  const X2YWs W = x2y_ws_layout(Nx, xdim, Ny, ydim, Hd, outdim, V);
  WsBound wb(workspace, W.split_floats);
  float* xk = saved + L.xk;
  float* xv = saved + L.xv;
  float* yq = saved + L.yq;
  float* feat = saved + L.feat;
  // keep X+Xpos / Y+Ypos for the weight gradients (basic.py:357-369); the position covers the first
  // *pos_cols channels (one launch either way)
  const float* xin = X;
  long long ldxin = ldx;
  if (Xpos) {
    FX_TRY(add2(X, ldx, Xpos, ldxp, Nx, xdim, saved + L.xin, xdim, 0, s, xpos_cols));
    xin = saved + L.xin;
    ldxin = xdim;
  }
  const float* yin = Y;
  long long ldyin = ldy;
  if (Ypos) {
    FX_TRY(add2(Y, ldy, Ypos, ldyp, Ny, ydim, saved + L.yin, ydim, 0, s, ypos_cols));
    yin = saved + L.yin;
    ldyin = ydim;
  }
  prof_begin(10, s);
  FX_TRY(linear_fwd(xin, ldxin, Nx, xdim, wk, bk, xk, Hd, Hd, 0, s));
  FX_TRY(linear_fwd(X, ldx, Nx, xdim, wv, bv, xv, Hd, Hd, 0, s));
  FX_TRY(linear_fwd(yin, ldyin, Ny, ydim, wq, bq, yq, Hd, Hd, 0, s));
  // algorithmic: the input rows, weights and outputs of the three products once
  prof_end(10, s, 2.0 * Hd * (2.0 * Nx * xdim + (double)Ny * ydim),
           4.0 * (2.0 * Nx * xdim + (double)Ny * ydim + Hd * (2.0 * xdim + ydim) + Hd * (2.0 * Nx + Ny)), 3);
  const float scale = 1.0f / std::sqrt((float)Hd);
  // a short key side (the a2f map: <= 320 action tokens per video): the whole core in one launch
  const bool al16 =
      ((reinterpret_cast<uintptr_t>(yq) | reinterpret_cast<uintptr_t>(xk) | reinterpret_cast<uintptr_t>(xv)) & 15) == 0;
  // algorithmic bytes of the attention core (bench roofline_attention): the query / key / value rows, the
  // logit and probability tiles, the attended features
  const double na = (double)V.a[V.n];
  const double core_bytes = 4.0 * ((double)Ny * Hd + 2.0 * Nx * Hd + 2.0 * na + (double)Ny * Hd);
  // fx_prof kinds 3 / 5 for frame-level calls, 11 / 13 for segment-level ones (bench.py reports them apart)
  const int kseg = std::max(Nx, Ny) >= 1024 ? 0 : 8;
  const int core = knobs().x2y_fused && al16 ? x2y_core_pick(V.n, V.x.data(), V.y.data(), Hd) : FX_X2Y_CORE_NONE;
  if (core == FX_X2Y_CORE_A2F || core == FX_X2Y_CORE_A2F_WIDE) {
    prof_begin(3 + kseg, s);
    FX_TRY(launch_x2y_a2f_fwd(yq, xk, xv, Hd, scale, V.n, V.y.data(), V.x.data(), V.a.data(), logit, attn, feat, s));
    prof_end(3 + kseg, s, 4.0 * na * Hd, core_bytes);
  } else if (core == FX_X2Y_CORE_F2A || core == FX_X2Y_CORE_F2A_WIDE) {
    // the f2a map (frames -> tokens): per-chunk partials after every other region of the workspace
    prof_begin(5 + kseg, s);
    FX_TRY(launch_x2y_f2a_fwd(yq, xk, xv, Hd, scale, V.n, V.y.data(), V.x.data(), V.a.data(), logit, attn, feat,
                              workspace + W.f2a, s));
    prof_end(5 + kseg, s, 4.0 * na * Hd, core_bytes);
  } else
  // per video: logits = scale yq . xk^T, attn = softmax(logits), feat = attn . xv  (the GEMMs of up to
  // two videos in one grouped launch each)
  for (int v0 = 0; v0 < V.n; v0 += 2) {
    fx_gemm_desc g1[2], g2[2];
    int n1 = 0, n2 = 0;
    for (int v = v0; v < std::min(V.n, v0 + 2); ++v) {
      const int nx = V.x[v + 1] - V.x[v], ny = V.y[v + 1] - V.y[v];
      if (nx == 0 || ny == 0) continue;
      fx_gemm_desc d = gemm_desc(ny, nx, Hd, op_rows(yq + (long long)V.y[v] * Hd, Hd),
                                 op_rows(xk + (long long)V.x[v] * Hd, Hd), logit + V.a[v], nx);
      d.alpha = scale;
      d.split_k = pick_split(ny, nx, Hd);
      d.workspace = workspace;
      g1[n1++] = d;
      d = gemm_desc(ny, Hd, nx, op_rows(attn + V.a[v], nx), op_cols(xv + (long long)V.x[v] * Hd, Hd),
                    feat + (long long)V.y[v] * Hd, Hd);
      d.split_k = pick_split(ny, Hd, nx);
      d.workspace = workspace;
      g2[n2++] = d;
    }
    FX_TRY(launch_gemm_group(g1, n1, s));
    for (int v = v0; v < std::min(V.n, v0 + 2); ++v) {
      const int nx = V.x[v + 1] - V.x[v], ny = V.y[v + 1] - V.y[v];
      if (nx == 0 || ny == 0) continue;
      FX_TRY(launch_softmax_rows(logit + V.a[v], nx, ny, nx, 1.f, attn + V.a[v], nx, s));
    }
    FX_TRY(launch_gemm_group(g2, n2, s));
  }
  // Y_W(cat[Y, feat]) with the concatenation folded into the A-operand loader; with dropout the
  // dropped concatenation is materialised (training only)
  fx_operand a = op_rows(Y, ldy);
  a.ptr1 = feat;
  a.ld1 = Hd;
  a.k_split = ydim;
  if (drop_p > 0.f) {
    float* catd = workspace + W.catd;
    FX_TRY(x2y_drop_cat(Y, ldy, feat, Ny, ydim, Hd, drop_p, seed, catd, s));
    a = op_rows(catd, ydim + Hd);
  }
  fx_gemm_desc d = gemm_desc(Ny, outdim, ydim + Hd, a, op_rows(wy, ydim + Hd), out, ldo);
  d.bias = by;
  return launch_gemm(d, s);
}

int fx_x2y_bwd(const float* X, long long ldx, int Nx, int xdim, int xpos_cols, const float* Y, long long ldy, int Ny,
               int ydim, int ypos_cols, const float* wk, const float* wv, const float* wq, const float* wy, int Hd,
               int outdim, int nvid, const int* x_off, const int* y_off, float drop_p, unsigned long long seed,
               const float* attn, const float* saved,
               const float* dout, long long lddo, const float* dlogit, const float* dattn, float* dX, float* dXpos,
               float* dY, float* dYpos, float* dwk, float* dbk, float* dwv, float* dbv, float* dwq, float* dbq,
               float* dwy, float* dby, int has_xpos, int has_ypos, float* workspace, int side_defer, int32_t* status,
               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const VidRows V = vid_rows(Nx, Ny, nvid, x_off, y_off);
  FX_REQUIRE(V.x[V.n] == Nx && V.y[V.n] == Ny, "x2y: offsets must end at Nx / Ny");
  const X2YLayout L = x2y_layout(Nx, xdim, Ny, ydim, Hd);
  const float* xk = saved + L.xk;
  const float* xv = saved + L.xv;
  const float* yq = saved + L.yq;
  const float* feat = saved + L.feat;
  const float* xin = has_xpos ? saved + L.xin : X;
  const long long ldxin = has_xpos ? xdim : ldx;
  const float* yin = has_ypos ? saved + L.yin : Y;
  const long long ldyin = has_ypos ? ydim : ldy;
  const int cw = ydim + Hd;
  const X2YWs W = x2y_ws_layout(Nx, xdim, Ny, ydim, Hd, outdim, V);
  float* dcat = workspace + W.dcat;
  float* dL = workspace + W.dL;
  float* dxv = workspace + W.dxv;
  float* dxk = workspace + W.dxk;
  float* dyq = workspace + W.dyq;
  float* dXk = workspace + W.dXk;
  float* dYq = workspace + W.dYq;
  float* spl = workspace + W.split;
  WsBound wb(spl, W.split_floats);
  const float scale = 1.0f / std::sqrt((float)Hd);
  // Y_W: dcat = dout . Wy, dWy = dout^T [Y, feat], dby  (dropout: the dropped concatenation and
  // the same mask on dcat)
  FX_TRY(linear_dx(dout, lddo, wy, Ny, cw, outdim, dcat, cw, 0, nullptr, 0, spl, s));
  const float* catd = nullptr;
  if (drop_p > 0.f) {
    float* cd = workspace + W.catd;
    FX_TRY(x2y_drop_cat(Y, ldy, feat, Ny, ydim, Hd, drop_p, seed, cd, s));
    FX_TRY(launch_dropout(dcat, cw, Ny, cw, cw, 0, drop_p, seed, dcat, cw, s));
    catd = cd;
  }
  // a short key side (the a2f map): dP, the softmax backward and dyq in one launch for every video; the
  // products that reduce over the query rows (dxv = attn^T dfeat, dxk = scale dlogit^T yq) stay
  // split-K GEMMs around it
  // the fused cores do float4 loads of the saved xk / xv / yq rows and of dcat: the same 16-B test as
  // the forward's (X2YLayout offsets Nx*xdim + Ny*ydim (+k*Nx*Hd) need not be multiples of 4 floats)
  const bool al16 = ((reinterpret_cast<uintptr_t>(xk) | reinterpret_cast<uintptr_t>(xv) |
                      reinterpret_cast<uintptr_t>(yq) | reinterpret_cast<uintptr_t>(dcat + ydim)) & 15) == 0;
  const int core = knobs().x2y_fused && (cw & 3) == 0 && al16 ? x2y_core_pick(V.n, V.x.data(), V.y.data(), Hd)
                                                                : FX_X2Y_CORE_NONE;
  const bool fused = core == FX_X2Y_CORE_A2F || core == FX_X2Y_CORE_A2F_WIDE;
  // algorithmic bytes of the backward core: dfeat, xv, xk, yq, attn (+ dattn / dlogit in), dlogit, dxv,
  // dxk, dyq out
  const double na = (double)V.a[V.n];
  const double core_bytes = 4.0 * (2.0 * Ny * Hd + 4.0 * Nx * Hd + 4.0 * na + (double)Ny * Hd);
  // the fused f2a core (bracketed as fx_prof kind 6 only when it runs: the per-video GEMM fallback below
  // is not the kernel whose algorithmic bytes kind 6 reports)
  const int f2a_mode = knobs().x2y_f2a_bwd;
  // (the wide f2a backward measured slower than the grouped GEMMs at every token count: FX_X2Y_F2A_BWD=1 only)
  const bool f2a_fused = (core == FX_X2Y_CORE_F2A || core == FX_X2Y_CORE_F2A_WIDE) &&
                         (f2a_mode == 1 || (f2a_mode == 2 && core == FX_X2Y_CORE_F2A &&
                                            x2y_f2a_chunks(V.n, V.x.data()) >= 64));
  const int kseg = std::max(Nx, Ny) >= 1024 ? 0 : 8;   // (fx_prof: frame-level 4 / 6, segment-level 12 / 14)
  if (fused) prof_begin(4 + kseg, s);
  else if (f2a_fused) prof_begin(6 + kseg, s);
  if (fused) {
    FX_TRY(launch_x2y_a2f_bwd(dcat + ydim, cw, xv, xk, attn, dattn, dlogit, Hd, scale, V.n, V.y.data(), V.x.data(),
                              V.a.data(), dL, dyq, s));
    // dxv = attn^T dfeat and dxk = scale dlogit^T yq: one launch over every video (x2y_a2f_dw_kernel), or
    // (FX_X2Y_A2F_DW=0) grouped split-K GEMMs of up to two videos per launch
    if (knobs().x2y_a2f_dw && x2y_a2f_dw_ok(V.n, V.y.data())) {
      FX_TRY(launch_x2y_a2f_dw(attn, dL, dcat + ydim, cw, yq, Hd, scale, V.n, V.y.data(), V.x.data(), V.a.data(), dxv,
                               dxk, spl, s));
    } else
    for (int v0 = 0; v0 < V.n; v0 += GMAX_GROUP / 2) {
      fx_gemm_desc g2[GMAX_GROUP];
      int n2 = 0;
      for (int v = v0; v < std::min(V.n, v0 + GMAX_GROUP / 2); ++v) {
        const int nx = V.x[v + 1] - V.x[v], ny = V.y[v + 1] - V.y[v];
        if (nx == 0 || ny == 0) continue;
        const long long xr = (long long)V.x[v] * Hd, yr = (long long)V.y[v] * Hd;
        fx_gemm_desc d = gemm_desc(nx, Hd, ny, op_cols(attn + V.a[v], nx),
                                   op_cols(dcat + (long long)V.y[v] * cw + ydim, cw), dxv + xr, Hd);
        d.split_k = pick_split(nx, Hd, ny);
        d.workspace = spl;
        g2[n2++] = d;
        d = gemm_desc(nx, Hd, ny, op_cols(dL + V.a[v], nx), op_cols(yq + yr, Hd), dxk + xr, Hd);
        d.alpha = scale;
        d.split_k = pick_split(nx, Hd, ny);
        d.workspace = spl;
        g2[n2++] = d;
      }
      FX_TRY(launch_gemm_group(g2, n2, s));
    }
  } else if (f2a_fused) {
    // the f2a map: dP / dxv, then dlogit / dxk / dyq partials per 64-key chunk, then the ordered dyq merge
    FX_TRY(launch_x2y_f2a_bwd(dcat + ydim, cw, xv, xk, yq, attn, dattn, dlogit, Hd, scale, V.n, V.y.data(), V.x.data(),
                              V.a.data(), dL, dxv, dxk, dyq, workspace + W.f2a, reinterpret_cast<unsigned*>(status), s));
  } else
  // per video: dP = dfeat . xv^T (+ dattn), dxv = attn^T . dfeat  (independent: one grouped launch
  // for up to two videos), softmax backward, then dyq = dlogit . xk, dxk = dlogit^T . yq (grouped)
  for (int v0 = 0; v0 < V.n; v0 += 2) {
    fx_gemm_desc g1[4], g2[4];
    int n1 = 0, n2 = 0;
    for (int v = v0; v < std::min(V.n, v0 + 2); ++v) {
      const int nx = V.x[v + 1] - V.x[v], ny = V.y[v + 1] - V.y[v];
      if (nx == 0 || ny == 0) continue;
      const float* dfeat = dcat + (long long)V.y[v] * cw + ydim;
      const float* at = attn + V.a[v];
      float* dl = dL + V.a[v];
      const long long xr = (long long)V.x[v] * Hd, yr = (long long)V.y[v] * Hd;
      fx_gemm_desc d = gemm_desc(ny, nx, Hd, op_rows(dfeat, cw), op_rows(xv + xr, Hd), dl, nx);
      d.resid = dattn ? dattn + V.a[v] : nullptr;
      d.ld_resid = nx;
      d.split_k = pick_split(ny, nx, Hd);
      d.workspace = spl;
      g1[n1++] = d;
      d = gemm_desc(nx, Hd, ny, op_cols(at, nx), op_cols(dfeat, cw), dxv + xr, Hd);
      d.split_k = pick_split(nx, Hd, ny);
      d.workspace = spl;
      g1[n1++] = d;
      d = gemm_desc(ny, Hd, nx, op_rows(dl, nx), op_cols(xk + xr, Hd), dyq + yr, Hd);
      d.alpha = scale;
      d.split_k = pick_split(ny, Hd, nx);
      d.workspace = spl;
      g2[n2++] = d;
      d = gemm_desc(nx, Hd, ny, op_cols(dl, nx), op_cols(yq + yr, Hd), dxk + xr, Hd);
      d.alpha = scale;
      d.split_k = pick_split(nx, Hd, ny);
      d.workspace = spl;
      g2[n2++] = d;
    }
    FX_TRY(launch_gemm_group(g1, n1, s));
    // dlogit = softmax_bwd(attn, dP) + dlogit_direct   (in place)
    for (int v = v0; v < std::min(V.n, v0 + 2); ++v) {
      const int nx = V.x[v + 1] - V.x[v], ny = V.y[v + 1] - V.y[v];
      if (nx == 0 || ny == 0) continue;
      float* dl = dL + V.a[v];
      FX_TRY(launch_softmax_rows_bwd(attn + V.a[v], nx, dl, nx, dlogit ? dlogit + V.a[v] : nullptr, nx, ny, nx, 1.f,
                                     dl, nx, s));
    }
    FX_TRY(launch_gemm_group(g2, n2, s));
  }
  if (fused) prof_end(4 + kseg, s, 8.0 * na * Hd, core_bytes);
  else if (f2a_fused) prof_end(6 + kseg, s, 8.0 * na * Hd, core_bytes);
  // weight gradients (Y_W; projections X_K, X_V, Y_Q): nothing below needs them -> side stream, each
  // frame-level GEMM split defer_split(rows) ways into its own slab region
  {
    const SideLane lane = side_lane(s);
    FX_TRY(lane.fork(1));
    float* sps = workspace + W.side;
    WsBound wbs(sps, W.side_floats);
    auto dw = [&](const float* dy, long long lddy, const float* x, long long ldx_, int rows, int K, int N, float* w,
                  float* b, long long ldw) -> int {
      fx_gemm_desc d = desc_linear_dwdb(dy, lddy, x, ldx_, rows, K, N, w, b, 1, sps, ldw);
      if (lane.ss) d.split_k = std::max(d.split_k, defer_split(rows));
      return launch_gemm(d, lane.side);
    };
    if (catd) {
      FX_TRY(dw(dout, lddo, catd, cw, Ny, cw, outdim, dwy, dby, cw));
    } else {
      FX_TRY(dw(dout, lddo, Y, ldy, Ny, ydim, outdim, dwy, dby, cw));
      FX_TRY(dw(dout, lddo, feat, Hd, Ny, Hd, outdim, dwy + ydim, nullptr, cw));
    }
    FX_TRY(dw(dxk, Hd, xin, ldxin, Nx, xdim, Hd, dwk, dbk, -1));
    FX_TRY(dw(dxv, Hd, X, ldx, Nx, xdim, Hd, dwv, dbv, -1));
    FX_TRY(dw(dyq, Hd, yin, ldyin, Ny, ydim, Hd, dwq, dbq, -1));
    FX_TRY(lane.join(side_defer));
  }
  if (dX || dXpos) {
    FX_TRY(linear_dx(dxk, Hd, wk, Nx, xdim, Hd, dXk, xdim, 0, nullptr, 0, spl, s));
    if (dXpos) FX_TRY(add2(dXk, xdim, nullptr, 0, Nx, xpos_cols, dXpos, xpos_cols, (has_xpos >> 1) & 1, s));
    if (dX) {
      fx_gemm_desc d = gemm_desc(Nx, xdim, Hd, op_rows(dxv, Hd), op_cols(wv, xdim), dX, xdim);
      d.resid = dXk;
      d.ld_resid = xdim;
      d.split_k = pick_split(Nx, xdim, Hd);
      d.workspace = spl;
      FX_TRY(launch_gemm(d, s));
    }
  }
  if (dY || dYpos) {
    FX_TRY(linear_dx(dyq, Hd, wq, Ny, ydim, Hd, dYq, ydim, 0, nullptr, 0, spl, s));
    if (dYpos) FX_TRY(add2(dYq, ydim, nullptr, 0, Ny, ypos_cols, dYpos, ypos_cols, (has_ypos >> 1) & 1, s));
    if (dY) FX_TRY(add2(dYq, ydim, dcat, cw, Ny, ydim, dY, ydim, 0, s));
  }
  return FX_OK;
}

}  // extern "C"
