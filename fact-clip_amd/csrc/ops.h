// Internal (non-ABI) declarations shared by the factmx translation units: the kernel files' launchers and
// the composite helpers of the host files (runtime.cpp, linear.cpp); frames.h adds what only the two MS-TCN
// files share.
#pragma once
#include "fx_common.h"

namespace fx {

// ---- kernels (rowops.hip, segments.hip, gru.hip, gemm_*.hip, attn_small.hip) ----
long long colsum_workspace_floats(int M, int N);
int launch_layernorm_fwd(const float* x, long long ldx, const float* r, long long ldr, const float* w,
                         const float* b, float eps, int rows, int cols, int relu, float* y, long long ldy,
                         float* mean, float* rstd, float* xhat, long long ldxh, hipStream_t s);
// the same, also writing y2 = y + pos (nullable: pos / y2 both or neither)
int launch_layernorm_fwd_pos(const float* x, long long ldx, const float* r, long long ldr, const float* w,
                             const float* b, float eps, int rows, int cols, int relu, float* y, long long ldy,
                             float* mean, float* rstd, float* xhat, long long ldxh, const float* pos, long long ldp,
                             float* y2, long long ldy2, hipStream_t s);
long long layernorm_bwd_ws_floats(int rows, int cols);
// LayerNorm weight / bias gradients of several LayerNorms in one launch: job j adds sum_rows dy * xhat to
// dw and sum_rows dy to db (either nullable), rows x cols, fixed row order (deterministic)
struct LnGradJob {
  const float* dy;
  const float* xhat;
  float* dw;
  float* db;
};
int launch_ln_param_grads(const LnGradJob* jobs, int n, int rows, int cols, long long lddy, long long ldxh,
                          hipStream_t s);
int launch_layernorm_bwd(const float* dy, long long lddy, const float* y, long long ldy, const float* xhat,
                         long long ldxh, const float* w, const float* rstd, int rows, int cols, int relu,
                         float* dx, long long lddx, float* dw, float* db, float* ws, hipStream_t s);
int launch_softmax_rows(const float* x, long long ldx, int rows, int cols, float scale, float* p, long long ldp,
                        hipStream_t s);
int launch_softmax_rows_bwd(const float* p, long long ldp, const float* dp, long long lddp, const float* extra,
                            long long lde, int rows, int cols, float scale, float* dl, long long ldd,
                            hipStream_t s);
int launch_pf_fwd(const float* x, long long ldx, int rows, int cols, int n, float* out, long long ldo, float* clogit,
                  long long ldc,
                  hipStream_t s);
int launch_pf_bwd(const float* out, long long ldo, const float* dout, long long lddo, const float* dcl,
                  long long lddc, int rows, int cols, int n, float* dx, long long lddx, hipStream_t s);
int launch_l2n_fwd(const float* x, long long ldx, int rows, int cols, float* y, long long ldy, float* nrm,
                   hipStream_t s);
int launch_l2n_bwd(const float* y, long long ldy, const float* nrm, const float* dy, long long lddy, int rows,
                   int cols, float* dx, long long lddx, hipStream_t s);
// nvid videos of T rows, or of the ragged host row offsets row_off (nvid + 1; NULL: uniform)
int launch_segments(const float* x, long long ldx, int col0, int ncls, int T, int nvid, const int* row_off,
                    int32_t* pred, int32_t* seg_id, int32_t* seg_start, int32_t* seg_end, int32_t* num_seg,
                    hipStream_t s);
// the two halves of launch_segments after its argmax, shared with the verb/noun argmax (verbnoun.hip):
// the row-layout checks (*rows = total rows) and the per-video boundary scan of pred
int segments_check_rows(int T, int nvid, const int* row_off, int* rows);
int launch_boundary_scan(const int32_t* pred, int T, int nvid, const int* row_off, int32_t* seg_id,
                         int32_t* seg_start, int32_t* seg_end, int32_t* num_seg, hipStream_t s);
// verb / noun class heads (verbnoun.hip; blocks_SepVerbNoun.py)
int launch_pf2_fwd(const float* x, long long ldx, int rows, int cols, int n1, int n2, float* out, long long ldo,
                   float* clogit, long long ldc, hipStream_t s);
int launch_pf2_bwd(const float* out, long long ldo, const float* dout, long long lddo, const float* dcl,
                   long long lddc, int rows, int cols, int n1, int n2, float* dx, long long lddx, hipStream_t s);
int launch_vn_logp_fwd(const float* clogit, long long ldc, int rows, int n1, int n2, const int32_t* vids,
                       const int32_t* nids, int A, int null, float* logp, long long ldl, float* lse, hipStream_t s);
int launch_vn_logp_bwd(const float* clogit, long long ldc, const float* lse, const float* dlogp, long long ldg,
                       int rows, int n1, int n2, int A, int null, const int32_t* voff, const int32_t* vlist,
                       const int32_t* noff, const int32_t* nlist, float* dclogit, long long lddc, hipStream_t s);
// the term table's FX_TERM_VNCLASS terms (vnloss.hip).  check_vn_terms: the host checks of those terms, their
// *count (0: neither launch below is made) and *lds_floats, the backward's dynamic LDS
int check_vn_terms(const fx_loss_term* terms_host, int nterms, bool bwd, int* count, long long* lds_floats);
void launch_vn_terms_fwd(const fx_loss_term* terms_dev, int nterms, float* part, hipStream_t s);
void launch_vn_terms_bwd(const fx_loss_term* terms_dev, int nterms, const float* gterm, long long lds_floats,
                         hipStream_t s);
int launch_segments_vn(const float* x, long long ldx, int col0, int n1, int n2, const int32_t* vids,
                       const int32_t* nids, int A, int T, int nvid, const int* row_off, int32_t* pred,
                       int32_t* seg_id, int32_t* seg_start, int32_t* seg_end, int32_t* num_seg, hipStream_t s);
int launch_seg_globalize(int nvid, int T, const int* row_off, const int32_t* num_seg_host, const int32_t* seg_id,
                         const int32_t* st, const int32_t* en, int32_t* gseg_id, int32_t* gst, int32_t* gen,
                         hipStream_t s);
int launch_seg_reduce(const float* x, long long ldx, const int32_t* st, const int32_t* en, int S, int cols, int mean,
                      float* y, long long ldy, int accumulate, hipStream_t s);
int launch_seg_mean_bwd(const float* dy, long long lddy, const int32_t* sid, const int32_t* st, const int32_t* en,
                        int T, int cols, float* dx, long long lddx, int accumulate, hipStream_t s);
// nseq independent sequences stacked by rows: sequence q owns rows [seq_off[q], seq_off[q+1]) (host)
int launch_gru_fwd(const float* gi, long long ldgi, int nseq, const int* seq_off, int Hh, const float* const whh[2],
                   const float* const bhh[2], float* out, long long ldo, int relu_out, float* saved, float* ws,
                   unsigned* status, int spin_max, hipStream_t s);
long long gru_sync_floats(int Hh, int nseq);
int launch_gru_bwd(const float* dout, long long lddo, const float* relu_y, long long ldy, int nseq, const int* seq_off,
                   int Hh, const float* const whh[2], const float* saved, float* dgi, long long lddgi, float* dgh,
                   float* sync_ws, unsigned* status, int spin_max, hipStream_t s);

// X2Y attention cores (x2y_a2f.hip, x2y_f2a.hip; shared device pieces: x2y_dev.h).  Token rows per video (keys of the a2f core, queries of the f2a core):
// <= 64 take the original kernels, 65 .. FX_X2Y_MAXTOK their wide variants (the launchers choose by the call's
// widest video); yoff / xoff: (nvid + 1) host row offsets, aoff: attention block offsets (ny_v * nx_v
// row-major each)
constexpr int FX_X2Y_MAXTOK = 320;
// which core a call takes -- the ONE decision behind fx_x2y_fwd, fx_x2y_bwd, fx_x2y_workspace_floats and
// fx_x2y_core (alignment and the FX_X2Y_* knobs aside)
enum { FX_X2Y_CORE_NONE = 0, FX_X2Y_CORE_A2F = 1, FX_X2Y_CORE_F2A = 2, FX_X2Y_CORE_A2F_WIDE = 3, FX_X2Y_CORE_F2A_WIDE = 4 };
int x2y_core_pick(int nvid, const int* xoff, const int* yoff, int Hd);
// short key side (a2f: <= 320 keys per video): logit, attn, feat in one launch;
// x2y_a2f_fusable / x2y_f2a_fusable: the <= 64-row conditions
bool x2y_a2f_fusable(int nvid, const int* xoff, int Hd);
int launch_x2y_a2f_fwd(const float* yq, const float* xk, const float* xv, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* logit, float* attn,
                       float* feat, hipStream_t s);
// long key side (f2a: <= 320 queries per video over up to T keys): chunk kernel + ordered merge; ws holds
// x2y_f2a_ws_floats(...) floats of per-chunk partials (slabs of 64 x the query blocks of the widest video)
bool x2y_f2a_fusable(int nvid, const int* xoff, const int* yoff, int Hd);
// 64-key chunks (= workgroups of the fused f2a backward passes) of a call
long long x2y_f2a_chunks(int nvid, const int* xoff);
long long x2y_f2a_ws_floats(int nvid, const int* xoff, const int* yoff, int Hd);
int launch_x2y_f2a_fwd(const float* yq, const float* xk, const float* xv, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* logit, float* attn,
                       float* feat, float* ws, hipStream_t s);
// f2a backward (dlogit, dxv, dxk, dyq of every video: the core in one launch with a grid barrier when every
// chunk's workgroup can be resident, else two, + the ordered dyq merge); ws as the forward's; status (nullable):
// FX_STATUS_X2Y_TIMEOUT when the one-launch core's barrier gives up
int launch_x2y_f2a_bwd(const float* dfeat, long long ldf, const float* xv, const float* xk, const float* yq,
                       const float* attn, const float* dattn, const float* dlogit_in, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* dlogit, float* dxv, float* dxk,
                       float* dyq, float* ws, unsigned* status, hipStream_t s);
// backward, input-gradient side: dP = dfeat . xv^T (+ dattn), dlogit = attn (dP - rowsum(attn dP)) (+ dlogit_in),
// dyq = scale dlogit . xk;  dfeat rows ld ldf (16-B aligned)
// the a2f backward's weight-side products dxv = attn^T dfeat, dxk = scale dlogit^T yq in one launch
// (x2y_a2f_dw_kernel; <= 320 keys per video, 64-key blocks of the output as a grid dimension);
// ws: x2y_a2f_dw_ws_floats(nvid, Hd, xoff) floats
long long x2y_a2f_dw_ws_floats(int nvid, int Hd, const int* xoff);
bool x2y_a2f_dw_ok(int nvid, const int* yoff);   // every video within the kernel's row chunks
int launch_x2y_a2f_dw(const float* attn, const float* dl, const float* dfeat, long long ldf, const float* yq, int Hd,
                      float scale, int nvid, const int* yoff, const int* xoff, const long long* aoff, float* dxv,
                      float* dxk, float* ws, hipStream_t s);
int launch_x2y_a2f_bwd(const float* dfeat, long long ldf, const float* xv, const float* xk, const float* attn,
                       const float* dattn, const float* dlogit_in, int Hd, float scale, int nvid, const int* yoff,
                       const int* xoff, const long long* aoff, float* dlogit, float* dyq, hipStream_t s);

// ---- composite helpers (runtime.cpp, linear.cpp) -------------------------------
// One entry point's use of the library's side stream (runtime.cpp): weight-gradient GEMMs that nothing
// downstream reads run on `side` while the input-gradient chain goes on on `main`.  Without a side stream
// (FX_SIDE_STREAM=0, or side_lane(main, false)) side == main and every call is a no-op.
struct SideStream;
struct SideLane {
  hipStream_t main, side;
  SideStream* ss;
  int fork(int e) const;          // side waits for main's work so far (fork event e: 0 .. 2)
  int done(int i) const;          // side: layer i's work is enqueued (event i & 3)
  int wait(int i) const;          // main waits for the side stream's layer i
  int join(bool deferred) const;  // main waits for all of side, unless the caller joins later (fx_side_join)
};
SideLane side_lane(hipStream_t main, bool on = true);

int ew_grid(long long total);
int relu_bwd(const float* dy, long long lddy, const float* y, long long ldy, int rows, int cols, float* dz,
             long long lddz, hipStream_t s);
// o (+)= a + b, b added on the first bcols columns only (bcols < 0: all)
int add2(const float* a, long long lda, const float* b, long long ldb, int rows, int cols, float* o, long long ldo,
         int accumulate, hipStream_t s, int bcols = -1);
// split-K factor / workspace floats for a (M x N, depth K) product
int pick_split(int M, int N, int K, int batch = 1);
long long split_ws(int M, int N, int K, int batch = 1);
// y = (x [+pos on the first pos_cols columns]) . w^T (+b) (+relu);  w (N,K) with row stride ldw
int linear_fwd(const float* x, long long ldx, int M, int K, const float* w, const float* b, float* y, long long ldy,
               int N, int relu, hipStream_t s, long long ldw = -1, const float* pos = nullptr, long long ldpos = 0,
               int pos_cols = 0);
// dx (+)= dy . w  [* (gate > 0)];  w (N,K)
int linear_dx(const float* dy, long long lddy, const float* w, int M, int K, int N, float* dx, long long lddx,
              int accumulate, const float* gate, long long ld_gate, float* ws, hipStream_t s, long long ldw = -1);
// dw (+)= dy^T . x and db (+)= colsum(dy) in one GEMM (virtual ones column)
int linear_dwdb(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N, float* dw,
                float* db, int accumulate, float* ws, hipStream_t s, long long lddw = -1);
int linear_dw(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N, float* dw,
              int accumulate, float* ws, hipStream_t s, long long lddw = -1);
long long dwdb_ws(int M, int K, int N);
// the same products as descriptors, for launch_gemm_group / linear_bwd_pair
fx_gemm_desc desc_linear_dx(const float* dy, long long lddy, const float* w, int M, int K, int N, float* dx,
                            long long lddx, int accumulate, const float* gate, long long ld_gate, float* ws,
                            long long ldw = -1);
fx_gemm_desc desc_linear_dwdb(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N,
                              float* dw, float* db, int accumulate, float* ws, long long lddw = -1);
// dW/db and dX of one linear layer from the same dY: one launch when both are direct-kernel shapes
int linear_bwd_pair(const fx_gemm_desc& dwdb, const fx_gemm_desc& dx, hipStream_t s);

// ---- fused small multi-head attention (attn_small.hip): Lq, Lk, head_dim <= 64 ----
// drop_p > 0: attention-probability dropout with the attention-over-T mask (TAttnOpts), probs saved un-dropped
// nvid independent problems stacked by rows (video v: q/o rows v*Lq.., k/v rows v*Lk..);
// probs (nvid, nhead, Lq, Lk) saved; o (Lq, nhead*hd) with row stride ldo.
// off (host, nvid + 1 row offsets from 0, self-attention): video v owns q/o and k/v rows [off[v], off[v+1]);
// Lq = Lk is then the longest video's count, the probs block of a video stays Lq * Lk per head (dense inside)
int launch_mha_small_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v,
                         long long ldv, int Lq, int Lk, int hd, int nhead, float scale, float* probs, float* o,
                         long long ldo, hipStream_t s, int nvid = 1, float drop_p = 0.f,
                         unsigned long long seed = 0, const int* off = nullptr);
// dq, dk, dv written (nullable) with their row strides
int launch_mha_small_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v,
                         long long ldv, const float* probs, const float* dout, long long lddo, int Lq, int Lk, int hd,
                         int nhead, float scale, float* dq, long long lddq, float* dk, long long lddk, float* dv,
                         long long lddv, hipStream_t s, int nvid = 1, float drop_p = 0.f, unsigned long long seed = 0,
                         const int* off = nullptr);

// ---- fused multi-head attention of queries over T frames (attention.cpp, attn_t_lds.hip, attn_t_rr.hip) ----
// nvid videos stacked by rows (queries v*Qv.., keys/values v*Tv.. or opt->koff); head h = columns
// [h*hd, h*hd+hd) of q/k/v/o.  fwd writes o and lse (nvid, nhead, Qv); bwd writes (or with acc_kv adds)
// dk, dv (rows: one per key) and writes dq.  More than 64 queries run as blocks of 64.
struct TAttnOpts {
  const int* koff = nullptr;        // host (nvid + 1) key-row offsets of ragged videos; Tv = the longest
  const int* qoff = nullptr;        // host (nvid + 1) query-row offsets of ragged videos; Qv = the longest
                                    // (lse then (nvid, nhead, Qv) with the longest video's stride)
  float drop_p = 0.f;               // attention-probability dropout (training)
  unsigned long long drop_seed = 0; // mask of probability (query row qg, head h, key row kg):
                                    // fx_drop_bits(seed, (qg * nhead + h) * total_key_rows + kg)
  int acc_kv = 0;                   // bwd: dk / dv += instead of =
};
long long tattn_ws_floats(int nvid, int Qv, int Tv, int hd, int nhead);
int launch_tattn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                     int nvid, int Qv, int Tv, int hd, int nhead, float scale, float* o, long long ldo, float* lse,
                     float* ws, hipStream_t s, const TAttnOpts* opt = nullptr);
int launch_tattn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                     const float* o, long long ldo, const float* dout, long long lddo, const float* lse, int nvid,
                     int Qv, int Tv, int hd, int nhead, float scale, float* dq, long long lddq, float* dk,
                     long long lddk, float* dv, long long lddv, float* ws, hipStream_t s,
                     const TAttnOpts* opt = nullptr);

// fused MS-TCN layer step (mstcn_fused.hip, per call: fx_mstcn_params.fused_layers): conv GEMM (K = 3F)
// -> row-local epilogue -> 1x1 GEMM; both weight matrices in the packed fragment order of
// launch_pack_frag (FN x K floats each)
bool frl_supported(int F, const void* x, long long ldx, long long ld_other);
// whether rows / 32 row tiles cover FX_FRL_MIN_FILL (80) % of the CUs of the current device: below that the
// fused layer leaves too many CUs idle and the two tuned GEMMs are faster (T = 2048 x 2 videos, 50 %: 11.6-11.8
// vs 12.0 ms per step; the shipped yaml's 4096 + 2900 rows, 86 %: the fused layer 0.5 ms faster)
// (min_fill_pct >= 0: that percentage instead of FX_FRL_MIN_FILL -- the MS-TCN++ layer's FX_FRL2_MIN_FILL)
bool frl_fills_device(long long rows, int min_fill_pct = -1);
long long frl_packed_floats(int K);
// one matrix [FN][K] (leading dim ld) -> fragment order at dst (frl_packed_floats(K) floats)
// (trans: the source is [K][FN], src[k * ld + n] -- the packed image is that of its transpose)
struct FragJob {
  const float* src;
  float* dst;
  int ld, K;
  int trans = 0;
};
constexpr int FRAG_JOBS = 48;   // matrices per pack launch
int launch_pack_frag(const FragJob* jobs, int n, hipStream_t s);
int launch_frl(const float* x, long long ldx, int M, int T, int dil, int dir, const int* seq_off, int nseq,
               const float* w1p, const float* bias1, int relu1, const float* resid1, long long ldr1, float* out1,
               long long ldo1, const float* w2p, const float* bias2, const float* resid2, long long ldr2,
               const float* gate2, long long ldg2, float* out2, long long ldo2, float drop_p,
               unsigned long long drop_seed, hipStream_t s, float vdrop_p = 0.f, unsigned long long vdrop_seed = 0,
               float* out3 = nullptr, long long ldo3 = 0);

// fused MS-TCN++ layer step (mstcn2_fused.hip, per call: fx_mstcn2_params.fused_layers), F = 256 rows as
// launch_frl's; every weight matrix in the packed fragment order of launch_pack_frag
struct Frl2Layer {
  int M, T;                       // rows; uniform videos of T rows (seq_off NULL)
  int dil1, dil2;                 // dilations of conv_d1 / conv_d2
  const int* seq_off;             // ragged videos: host (nseq + 1) row offsets, <= 16 videos
  int nseq;
  float drop_p;                   // fwd: layer i's dropout on r_i; bwd: layer i - 1's, on G_i as dU_i-1 reads it
  unsigned long long drop_seed;   // fx_drop_subseed(seed, that layer)
};
// cat = [conv_d1(f) + b1 | conv_d2(f) + b2] (ld 2F), r = dropout(relu(cat . W_fu^T + bfu)), fnext = f + r;
// w1p / w2p: the forward conv images (K = 3F), wfup: W_fu (K = 2F)
int launch_frl2_fwd(const Frl2Layer& y, const float* f, const float* w1p, const float* w2p, const float* b1,
                    const float* b2, float* cat, const float* wfup, const float* bfu, float* r, float* fnext,
                    hipStream_t s);
// gout = gnext + conv_d1^T(dcat[:, 0:F]) + conv_d2^T(dcat[:, F:2F]), du = dropout(gout) * (rprev > 0),
// dcat_prev = du . W_fu (ld 2F);  wb1p / wb2p: the dX conv images (K = 3F), wfutp: the two halves of W_fu^T
// (K = F each, half h at h F F)
int launch_frl2_bwd(const Frl2Layer& y, const float* dcat, const float* wb1p, const float* wb2p, const float* gnext,
                    float* gout, const float* rprev, float* du, const float* wfutp, float* dcat_prev, hipStream_t s);

// ---- grouped dilated Conv1d(k = 3) (conv_grouped.hip): nn.Conv1d(F, F, 3, groups = ngroup), cg = F / ngroup ----
// Videos: nvid of T rows (rows = T * nvid) or the ragged host row offsets seq_off (nvid + 1, <= 16 videos);
// a shifted row outside its video reads as zero.  Always on the f32 MFMA, whatever the precision mode.
int gconv_check(int F, int ngroup, const char* who);   // ngroup >= 0 and F % max(ngroup, 1) == 0, else FX_ERR_SHAPE
long long gconv_packed_floats(int F, int ngroup);      // 3 F cg: one packed image
// (F, cg, 3) -> wf [q][tap][n][c] (forward) and wb [q][tap][c][n] (input gradient); optionally a 1x1 weight
// wpw (F, F) -> wpt transposed
struct GPackJob {
  const float* w;
  float* wf;
  float* wb;
  const float* wpw;
  float* wpt;
};
int launch_gconv_pack(const GPackJob* jobs, int n, int F, int ngroup, hipStream_t s);
// y (+)= act(conv(x; wp) + bias) (+ resid): dir = 1 over the wf image is the forward, dir = -1 over wb the input
// gradient; bias / resid nullable
int launch_gconv(const float* x, long long ldx, int rows, int T, int nvid, const int* seq_off, int F, int ngroup,
                 int dil, int dir, const float* wp, const float* bias, int relu, const float* resid, long long ldr,
                 int accumulate, float* y, long long ldy, hipStream_t s);
// dw (F, cg, 3) += dz^T taps(x), db (F) += colsum(dz) (either nullable): split-K partials in ws
// (gconv_dw_ws_floats), reduced in split order -- deterministic, no atomics
long long gconv_dw_ws_floats(int rows, int F, int ngroup);
int launch_gconv_dw(const float* dz, long long lddz, const float* x, long long ldx, int rows, int T, int nvid,
                    const int* seq_off, int F, int ngroup, int dil, float* dw, float* db, float* ws, hipStream_t s);

}  // namespace fx
