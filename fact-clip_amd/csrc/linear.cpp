// Linear layers and element-wise helpers: the split-K planner, the linear_* / desc_linear_* products the
// composite ops are built from, and the entry points that are one call into a kernel file (GEMM, dropout,
// row ops, verb / noun heads, GRU, segments).
#include <algorithm>
#include <vector>

#include "fx_common.h"
#include "ops.h"

namespace fx {
namespace {

__global__ void relu_bwd_kernel(const float* dy, long long lddy, const float* y, long long ldy, int rows, int cols,
                                float* dz, long long lddz) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cols, c = i % cols;
    dz[r * lddz + c] = y[r * ldy + c] > 0.f ? dy[r * lddy + c] : 0.f;
  }
}

__global__ void add2_kernel(const float* a, long long lda, const float* b, long long ldb, int rows, int cols,
                            float* o, long long ldo, int accumulate, int bcols) {
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cols, c = i % cols;
    const float v = a[r * lda + c] + (b && c < bcols ? b[r * ldb + c] : 0.f);
    o[r * ldo + c] = accumulate ? o[r * ldo + c] + v : v;
  }
}

}  // namespace

int ew_grid(long long total) { return (int)std::min<long long>(std::max<long long>(cdiv(total, 256), 1), 4096); }

int relu_bwd(const float* dy, long long lddy, const float* y, long long ldy, int rows, int cols, float* dz,
             long long lddz, hipStream_t s) {
  if ((long long)rows * cols == 0) return FX_OK;
  fx_launch(relu_bwd_kernel, dim3(ew_grid((long long)rows * cols)), dim3(256), 0, s, dy, lddy, y, ldy, rows,
                     cols, dz, lddz);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int add2(const float* a, long long lda, const float* b, long long ldb, int rows, int cols, float* o, long long ldo,
         int accumulate, hipStream_t s, int bcols) {
  if ((long long)rows * cols == 0) return FX_OK;
  fx_launch(add2_kernel, dim3(ew_grid((long long)rows * cols)), dim3(256), 0, s, a, lda, b, ldb, rows, cols,
                     o, ldo, accumulate, bcols < 0 ? cols : bcols);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

// split-K factor for small-output / long-K products (dW over frames, token x frame)
int pick_split(int M, int N, int K, int batch) {
  const int nkt = cdiv(K, 64);   // 64-deep K stages of the GEMM kernel
  if (nkt < 4) return 1;
  // whole 64-deep stages and >= 128 rows: the launch can take the 128x64 tile (8 waves), so count
  // those tiles; one block per CU: keep tiles*split within the 256 CUs, no straggler round
  const bool wide = M >= 128 && K % 64 == 0;
  const long long tiles = (long long)cdiv(M, wide ? 128 : 64) * cdiv(N, 64) * batch;
  if (tiles >= 160) return 1;
  int sp = (int)std::min<long long>(nkt / 2, 256 / tiles);
  return std::max(sp, 1);
}

long long split_ws(int M, int N, int K, int batch) {
  const int sp = pick_split(M, N, K, batch);
  return sp > 1 ? (long long)sp * M * N * batch : 0;
}

// y = (x [+pos on the first pos_cols columns]) . w^T (+b) (+relu);  w (N,K) with row stride ldw
int linear_fwd(const float* x, long long ldx, int M, int K, const float* w, const float* b, float* y, long long ldy,
               int N, int relu, hipStream_t s, long long ldw, const float* pos, long long ldpos, int pos_cols) {
  fx_gemm_desc d = gemm_desc(M, N, K, op_rows(x, ldx), op_rows(w, ldw < 0 ? K : ldw), y, ldy);
  d.a.pos = pos;
  d.a.ld_pos = ldpos;
  d.a.pos_cols = pos ? pos_cols : 0;
  d.bias = b;
  d.relu = relu;
  return launch_gemm(d, s);
}

// dx (+)= dy . w  [* (gate > 0)];  w (N,K)
fx_gemm_desc desc_linear_dx(const float* dy, long long lddy, const float* w, int M, int K, int N, float* dx,
                            long long lddx, int accumulate, const float* gate, long long ld_gate, float* ws,
                            long long ldw) {
  fx_gemm_desc d = gemm_desc(M, K, N, op_rows(dy, lddy), op_cols(w, ldw < 0 ? K : ldw), dx, lddx);
  d.beta = accumulate ? 1.f : 0.f;
  d.gate = gate;
  d.ld_gate = ld_gate;
  d.split_k = pick_split(M, K, N);
  d.workspace = ws;
  return d;
}

int linear_dx(const float* dy, long long lddy, const float* w, int M, int K, int N, float* dx, long long lddx,
              int accumulate, const float* gate, long long ld_gate, float* ws, hipStream_t s, long long ldw) {
  return launch_gemm(desc_linear_dx(dy, lddy, w, M, K, N, dx, lddx, accumulate, gate, ld_gate, ws, ldw), s);
}

// dw (+)= dy^T . x  and  db (+)= colsum(dy)  in ONE GEMM: x gets a virtual all-ones column K
// whose output column (the bias gradient) is routed to db.  dy (M,N), x (M,K) -> dw (N,K), ld lddw.
// (no dw and no db: an empty desc, M = 0, that launch_gemm / launch_gemm_group skip)
fx_gemm_desc desc_linear_dwdb(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N,
                              float* dw, float* db, int accumulate, float* ws, long long lddw) {
  if (!dw) {
    fx_gemm_desc e{};
    e.batch = 1;
    e.c_last_col = db;   // (a bias-only request: linear_bwd_pair refuses it like linear_dwdb)
    return e;
  }
  fx_operand b = op_cols(x, ldx);
  const int Kc = K + (db ? 1 : 0);
  if (db) b.ones_col = K + 1;
  fx_gemm_desc d = gemm_desc(N, Kc, M, op_cols(dy, lddy), b, dw, lddw < 0 ? K : lddw);
  d.c_last_col = db;
  d.beta = accumulate ? 1.f : 0.f;
  // split sized for the K+1 columns dwdb_ws() reserves, with or without the bias column: counting
  // only K columns can pick a larger split (fewer tiles) than the reservation holds
  d.split_k = pick_split(N, K + 1, M);
  d.workspace = ws;
  return d;
}

int linear_dwdb(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N, float* dw,
                float* db, int accumulate, float* ws, hipStream_t s, long long lddw) {
  if (!dw && !db) return FX_OK;
  FX_REQUIRE(dw, "linear_dwdb: bias-only gradient needs dw");
  return launch_gemm(desc_linear_dwdb(dy, lddy, x, ldx, M, K, N, dw, db, accumulate, ws, lddw), s);
}

// The two independent backward GEMMs of one linear layer (dW/db = dY^T X, dX = dY W): one launch
// when both take the direct kernel (token-level shapes), else two.
int linear_bwd_pair(const fx_gemm_desc& dwdb, const fx_gemm_desc& dx, hipStream_t s) {
  FX_REQUIRE(!(dwdb.c_last_col && !dwdb.c), "linear_dwdb: bias-only gradient needs dw");
  const fx_gemm_desc pr[2] = {dwdb, dx};
  return launch_gemm_group(pr, 2, s);
}

int linear_dw(const float* dy, long long lddy, const float* x, long long ldx, int M, int K, int N, float* dw,
              int accumulate, float* ws, hipStream_t s, long long lddw) {
  return linear_dwdb(dy, lddy, x, ldx, M, K, N, dw, nullptr, accumulate, ws, s, lddw);
}

long long dwdb_ws(int M, int K, int N) { return split_ws(N, K + 1, M); }

// Split of the deferred batched weight-gradient GEMMs (fx_mstcn_bwd, fx_x2y_bwd): each workgroup of a batched
// launch otherwise walks all K = rows and holds its CU for the whole launch, so the main stream's
// next kernels wait for CUs; 16 caps a workgroup's share at K / 16 (16 vs 8: 15.78 vs 15.95 ms, median
// of 6 pairs, round 3)
#ifndef FX_DEFER_SPLIT_BUILD
#define FX_DEFER_SPLIT_BUILD 16   // (a diagnostic build define for A/B runs)
#endif
int defer_split(int rows) { return std::max(1, std::min(FX_DEFER_SPLIT_BUILD, rows / 512)); }

}  // namespace fx

using namespace fx;

extern "C" {

int fx_dropout(const float* x, long long ldx, int rows, int cols, long long idx_ld, long long idx_col0, float p,
               unsigned long long seed, float* y, long long ldy, void* stream) {
  FX_REQUIRE(x && y && rows >= 0 && cols >= 0, "dropout: bad arguments");
  return launch_dropout(x, ldx, rows, cols, idx_ld, idx_col0, p, seed, y, ldy, (hipStream_t)stream);
}

int fx_gemm(const fx_gemm_desc* desc, void* stream) {
  FX_REQUIRE(desc, "fx_gemm: null descriptor");
  // implicit dilated-conv GEMMs (A = shifted-tap operand: conv forward / conv dX, e.g. MSTCN2) are
  // the same kernel class the bench times inside fx_mstcn_*
  const bool conv = desc->a.conv_taps && !desc->a.trans;
  if (conv) prof_begin(0, (hipStream_t)stream);
  const int st = launch_gemm(*desc, (hipStream_t)stream);
  if (conv) prof_end(0, (hipStream_t)stream, 2.0 * desc->M * desc->N * desc->K * desc->batch, 0.0);
  return st;
}

long long fx_gemm_workspace_floats(const fx_gemm_desc* desc) { return desc ? gemm_workspace_floats(*desc) : 0; }

// ---------------------------------------------------------------- Linear
int fx_linear_fwd(const float* x, long long ldx, const float* pos, long long ldpos, int pos_cols, int M, int K,
                  const float* w, long long ldw, const float* b, float* y, long long ldy, int N, int relu,
                  void* stream) {
  return linear_fwd(x, ldx, M, K, w, b, y, ldy, N, relu, (hipStream_t)stream, ldw, pos, ldpos, pos_cols);
}

long long fx_linear_bwd_workspace_floats(int M, int K, int N) {
  return (long long)M * N + split_ws(M, K, N) + dwdb_ws(M, K, N) + colsum_workspace_floats(M, N);
}

int fx_linear_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* w, long long ldw,
                  const float* relu_out, long long ld_relu, int M, int K, int N, float* dx, long long lddx,
                  float* dw, long long lddw, float* db, int accumulate_dx, int accumulate_w, float* workspace,
                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(workspace || (!relu_out && split_ws(M, K, N) == 0 && dwdb_ws(M, K, N) == 0 && !(db && !dw)),
             "fx_linear_bwd: workspace required");
  float* wz = workspace;
  float* wsx = wz + (long long)M * N;
  float* wsw = wsx + split_ws(M, K, N);
  float* wsc = wsw + dwdb_ws(M, K, N);
  const float* g = dy;
  long long ldg = lddy;
  if (relu_out) {
    FX_TRY(relu_bwd(dy, lddy, relu_out, ld_relu, M, N, wz, N, s));
    g = wz;
    ldg = N;
  }
  if (dx) {
    WsBound wb(wsx, split_ws(M, K, N));
    FX_TRY(linear_dx(g, ldg, w, M, K, N, dx, lddx, accumulate_dx, nullptr, 0, wsx, s, ldw));
  }
  if (dw) {
    WsBound wb(wsw, dwdb_ws(M, K, N));
    FX_TRY(linear_dwdb(g, ldg, x, ldx, M, K, N, dw, db, accumulate_w, wsw, s, lddw));
  }
  else if (db) FX_TRY(launch_colsum(g, ldg, M, N, db, accumulate_w, wsc, s));
  return FX_OK;
}

// ---------------------------------------------------------------- row ops
int fx_layernorm_fwd(const float* x, long long ldx, const float* r, long long ldr, const float* w, const float* b,
                     float eps, int rows, int cols, int relu, float* y, long long ldy, float* xhat, long long ldxh,
                     float* rstd, void* stream) {
  return launch_layernorm_fwd(x, ldx, r, ldr, w, b, eps, rows, cols, relu, y, ldy, nullptr, rstd, xhat, ldxh,
                              (hipStream_t)stream);
}

long long fx_layernorm_bwd_workspace_floats(int rows, int cols) { return layernorm_bwd_ws_floats(rows, cols); }

int fx_layernorm_bwd(const float* dy, long long lddy, const float* y, long long ldy, const float* xhat,
                     long long ldxh, const float* w, const float* rstd, int rows, int cols, int relu, float* dx,
                     long long lddx, float* dw, float* db, float* workspace, void* stream) {
  return launch_layernorm_bwd(dy, lddy, y, ldy, xhat, ldxh, w, rstd, rows, cols, relu, dx, lddx, dw, db, workspace,
                              (hipStream_t)stream);
}

int fx_softmax_rows(const float* logits, long long ldl, int rows, int cols, float scale, float* probs,
                    long long ldp, void* stream) {
  return launch_softmax_rows(logits, ldl, rows, cols, scale, probs, ldp, (hipStream_t)stream);
}

int fx_softmax_rows_bwd(const float* probs, long long ldp, const float* dprobs, long long lddp,
                        const float* dlogit_extra, long long lde, int rows, int cols, float scale, float* dlogit,
                        long long ldd, void* stream) {
  return launch_softmax_rows_bwd(probs, ldp, dprobs, lddp, dlogit_extra, lde, rows, cols, scale, dlogit, ldd,
                                 (hipStream_t)stream);
}

int fx_process_feature_fwd(const float* x, long long ldx, int rows, int cols, int n, float* out, long long ldo,
                           float* clogit, long long ldc, void* stream) {
  return launch_pf_fwd(x, ldx, rows, cols, n, out, ldo, clogit, ldc, (hipStream_t)stream);
}

int fx_process_feature_bwd(const float* out, long long ldo, const float* dout, long long lddo, const float* dclogit,
                           long long lddc, int rows, int cols, int n, float* dx, long long lddx, void* stream) {
  return launch_pf_bwd(out, ldo, dout, lddo, dclogit, lddc, rows, cols, n, dx, lddx, (hipStream_t)stream);
}

// ---------------------------------------------------------------- verb / noun class heads (verbnoun.hip)
int fx_process_feature2_fwd(const float* x, long long ldx, int rows, int cols, int n1, int n2, float* out,
                            long long ldo, float* clogit, long long ldc, void* stream) {
  return launch_pf2_fwd(x, ldx, rows, cols, n1, n2, out, ldo, clogit, ldc, (hipStream_t)stream);
}

int fx_process_feature2_bwd(const float* out, long long ldo, const float* dout, long long lddo, const float* dclogit,
                            long long lddc, int rows, int cols, int n1, int n2, float* dx, long long lddx,
                            void* stream) {
  return launch_pf2_bwd(out, ldo, dout, lddo, dclogit, lddc, rows, cols, n1, n2, dx, lddx, (hipStream_t)stream);
}

int fx_vn_logp_fwd(const float* clogit, long long ldc, int rows, int n1, int n2, const int32_t* vids,
                   const int32_t* nids, int A, int null, float* logp, long long ldl, float* lse, void* stream) {
  return launch_vn_logp_fwd(clogit, ldc, rows, n1, n2, vids, nids, A, null, logp, ldl, lse, (hipStream_t)stream);
}

int fx_vn_logp_bwd(const float* clogit, long long ldc, const float* lse, const float* dlogp, long long ldg, int rows,
                   int n1, int n2, int A, int null, const int32_t* voff, const int32_t* vlist, const int32_t* noff,
                   const int32_t* nlist, float* dclogit, long long lddc, void* stream) {
  return launch_vn_logp_bwd(clogit, ldc, lse, dlogp, ldg, rows, n1, n2, A, null, voff, vlist, noff, nlist, dclogit,
                            lddc, (hipStream_t)stream);
}

int fx_segments_from_vn_probs(const float* x, long long ldx, int col0, int n1, int n2, const int32_t* vids,
                              const int32_t* nids, int A, int T, int nvid, const int* row_off, int32_t* pred,
                              int32_t* seg_id, int32_t* seg_start, int32_t* seg_end, int32_t* num_seg, void* stream) {
  return launch_segments_vn(x, ldx, col0, n1, n2, vids, nids, A, T, nvid, row_off, pred, seg_id, seg_start, seg_end,
                            num_seg, (hipStream_t)stream);
}

int fx_l2norm_fwd(const float* x, long long ldx, int rows, int cols, float* y, long long ldy, float* norm,
                  void* stream) {
  return launch_l2n_fwd(x, ldx, rows, cols, y, ldy, norm, (hipStream_t)stream);
}

int fx_l2norm_bwd(const float* y, long long ldy, const float* norm, const float* dy, long long lddy, int rows,
                  int cols, float* dx, long long lddx, void* stream) {
  return launch_l2n_bwd(y, ldy, norm, dy, lddy, rows, cols, dx, lddx, (hipStream_t)stream);
}

int fx_relu_bwd(const float* dy, long long lddy, const float* y, long long ldy, int rows, int cols, float* dz,
                long long lddz, void* stream) {
  return relu_bwd(dy, lddy, y, ldy, rows, cols, dz, lddz, (hipStream_t)stream);
}

int fx_add(const float* a, long long lda, const float* b, long long ldb, int rows, int cols, float* out,
           long long ldo, int accumulate, void* stream) {
  return add2(a, lda, b, ldb, rows, cols, out, ldo, accumulate, (hipStream_t)stream);
}

// ---------------------------------------------------------------- bidirectional GRU
long long fx_gru_saved_floats(int S, int Hh) { return 10LL * S * Hh; }

static long long gru_split_ws(int S, int In, int Hh) {
  long long sp = std::max(dwdb_ws(S, In, 3 * Hh), dwdb_ws(S, Hh, 3 * Hh));
  return std::max(sp, split_ws(S, In, 3 * Hh));
}

// Offset of the backward's sync area, rounded up to an even number of floats: its granules are 8-byte atomics,
// and with an odd Hh the tables before it hold an odd number of floats (a granule straddling two 4-byte words
// is stored and polled in halves, so a reader can pair the new epoch with the previous step's value)
static long long gru_bwd_sync_off(int S, int In, int Hh) {
  const long long H3 = 3LL * Hh;
  const long long n = S * 2 * H3 + 2 * S * H3 + gru_split_ws(S, In, Hh) + colsum_workspace_floats(S, 3 * Hh);
  return (n + 1) & ~1LL;
}

// fwd: [sync area][gi (S, 6Hh)];  bwd: [dgi (S, 6Hh)][dgh 2 x (S, 3Hh)][split-K][colsum][pad to 8 B][sync area]
long long fx_gru_workspace_floats(int S, int nseq, int In, int Hh) {
  const long long H3 = 3LL * Hh;
  long long fwd = gru_sync_floats(Hh, nseq) + S * 2 * H3;
  long long bwd = gru_bwd_sync_off(S, In, Hh) + gru_sync_floats(Hh, nseq);
  return std::max(fwd, bwd);
}

static std::vector<int> seq_offsets(int S, int nseq, const int* seq_off) {
  if (nseq <= 1 || !seq_off) return {0, S};
  return std::vector<int>(seq_off, seq_off + nseq + 1);
}

int fx_gru_bidir_fwd(const float* x, long long ldx, int S, int nseq, const int* seq_off, int In, int Hh,
                     const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f,
                     const float* w_ih_r, const float* w_hh_r, const float* b_ih_r, const float* b_hh_r, float* out,
                     long long ldo, int relu_out, float* saved, float* workspace, int32_t* status, int spin_max,
                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int H3 = 3 * Hh;
  const std::vector<int> off = seq_offsets(S, nseq, seq_off);
  const int nq = (int)off.size() - 1;
  FX_REQUIRE(off.back() == S && off.front() == 0, "gru: sequence offsets must span [0, S]");
  float* gi = workspace + gru_sync_floats(Hh, nq);
  // input projections of every step, both directions: gi[:, d*3Hh:(d+1)*3Hh] = x W_ih_d^T + b_ih_d
  FX_TRY(linear_fwd(x, ldx, S, In, w_ih_f, b_ih_f, gi, 2 * H3, H3, 0, s));
  FX_TRY(linear_fwd(x, ldx, S, In, w_ih_r, b_ih_r, gi + H3, 2 * H3, H3, 0, s));
  const float* whh[2] = {w_hh_f, w_hh_r};
  const float* bhh[2] = {b_hh_f, b_hh_r};
  return launch_gru_fwd(gi, 2 * H3, nq, off.data(), Hh, whh, bhh, out, ldo, relu_out, saved, workspace,
                        (unsigned*)status, spin_max, s);
}

int fx_gru_bidir_bwd(const float* x, long long ldx, int S, int nseq, const int* seq_off, int In, int Hh,
                     const float* w_ih_f, const float* w_hh_f, const float* w_ih_r, const float* w_hh_r,
                     const float* saved, const float* dout, long long lddo, const float* relu_y, long long ldy,
                     float* dx, long long lddx, float* dw_ih_f,
                     float* dw_hh_f, float* db_ih_f, float* db_hh_f, float* dw_ih_r, float* dw_hh_r, float* db_ih_r,
                     float* db_hh_r, float* workspace, int32_t* status, int spin_max, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int H3 = 3 * Hh;
  const std::vector<int> off = seq_offsets(S, nseq, seq_off);
  const int nq = (int)off.size() - 1;
  FX_REQUIRE(off.back() == S && off.front() == 0, "gru: sequence offsets must span [0, S]");
  float* dgi = workspace;                          // (S, 6Hh)
  float* dgh = dgi + (long long)S * 2 * H3;        // 2 x (S, 3Hh)
  float* spl = dgh + 2LL * S * H3;
  float* csw = spl + gru_split_ws(S, In, Hh);
  WsBound wb(spl, gru_split_ws(S, In, Hh));
  float* sync_ws = workspace + gru_bwd_sync_off(S, In, Hh);
  const float* whh[2] = {w_hh_f, w_hh_r};
  FX_TRY(launch_gru_bwd(dout, lddo, relu_y, ldy, nq, off.data(), Hh, whh, saved, dgi, 2 * H3, dgh, sync_ws,
                        (unsigned*)status, spin_max, s));
  const float* wih[2] = {w_ih_f, w_ih_r};
  float* dwih[2] = {dw_ih_f, dw_ih_r};
  float* dwhh[2] = {dw_hh_f, dw_hh_r};
  float* dbih[2] = {db_ih_f, db_ih_r};
  float* dbhh[2] = {db_hh_f, db_hh_r};
  for (int d = 0; d < 2; ++d) {
    const float* gi_d = dgi + d * H3;
    const float* gh_d = dgh + (long long)d * S * H3;
    const float* hp_d = saved + (long long)d * S * Hh;
    if (dwih[d]) FX_TRY(linear_dwdb(gi_d, 2 * H3, x, ldx, S, In, H3, dwih[d], dbih[d], 1, spl, s));
    else if (dbih[d]) FX_TRY(launch_colsum(gi_d, 2 * H3, S, H3, dbih[d], 1, csw, s));
    if (dwhh[d]) FX_TRY(linear_dwdb(gh_d, H3, hp_d, Hh, S, Hh, H3, dwhh[d], dbhh[d], 1, spl, s));
    else if (dbhh[d]) FX_TRY(launch_colsum(gh_d, H3, S, H3, dbhh[d], 1, csw, s));
    if (dx) FX_TRY(linear_dx(gi_d, 2 * H3, wih[d], S, In, H3, dx, lddx, d, nullptr, 0, spl, s));
  }
  return FX_OK;
}

// ---------------------------------------------------------------- segments
int fx_segments_from_probs(const float* x, long long ldx, int col0, int ncls, int T, int nvid, const int* row_off,
                           int32_t* pred, int32_t* seg_id, int32_t* seg_start, int32_t* seg_end, int32_t* num_seg,
                           void* stream) {
  return launch_segments(x, ldx, col0, ncls, T, nvid, row_off, pred, seg_id, seg_start, seg_end, num_seg,
                         (hipStream_t)stream);
}

int fx_segments_globalize(int nvid, int T, const int* row_off, const int32_t* num_seg_host, const int32_t* seg_id,
                          const int32_t* seg_start, const int32_t* seg_end, int32_t* gseg_id, int32_t* gstart,
                          int32_t* gend, void* stream) {
  FX_REQUIRE(nvid >= 1 && (T > 0 || row_off) && num_seg_host, "segments_globalize: bad arguments");
  return launch_seg_globalize(nvid, T, row_off, num_seg_host, seg_id, seg_start, seg_end, gseg_id, gstart, gend,
                              (hipStream_t)stream);
}

int fx_seg_mean_fwd(const float* x, long long ldx, const int32_t* seg_start, const int32_t* seg_end, int S, int cols,
                    float* y, long long ldy, void* stream) {
  return launch_seg_reduce(x, ldx, seg_start, seg_end, S, cols, 1, y, ldy, 0, (hipStream_t)stream);
}

int fx_seg_mean_bwd(const float* dy, long long lddy, const int32_t* seg_id, const int32_t* seg_start,
                    const int32_t* seg_end, int T, int cols, float* dx, long long lddx, int accumulate, void* stream) {
  return launch_seg_mean_bwd(dy, lddy, seg_id, seg_start, seg_end, T, cols, dx, lddx, accumulate, (hipStream_t)stream);
}

int fx_seg_sum_rows(const float* dx, long long lddx, const int32_t* seg_start, const int32_t* seg_end, int S, int cols,
                    float* dy, long long lddy, int accumulate, void* stream) {
  return launch_seg_reduce(dx, lddx, seg_start, seg_end, S, cols, 0, dy, lddy, accumulate, (hipStream_t)stream);
}

}  // extern "C"
