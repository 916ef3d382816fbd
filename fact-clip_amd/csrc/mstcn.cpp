// MS-TCN stack: layout of its saved activations and workspace, forward, and the four backward schedules.
#include <algorithm>
#include <vector>

#include "fx_common.h"
#include "ops.h"
#include "frames.h"

namespace fx {
namespace {

struct PackArgs {
  const float* w[32];
  float* wf[32];
  float* wb[32];
  const float* wpw[32];   // 1x1 weights (F_out, F_in) -> wpt = transposed (fused backward chain)
  float* wpt[32];
  int F;
};

// Conv1d weight (F_out=F, F_in=F, 3) -> Wf[n][j*F+c] (forward B) and Wb[c][j*F+n] (dX B);
// 1x1 weight W[o][c] -> Wt[c][o].  One 32 (out) x 32 (in) x 3 (tap) tile per workgroup through LDS:
// coalesced reads of the (F, F, 3) rows and coalesced 32-float writes of both packed images (the
// element-wise version scattered every Wb write: 85 us per 10-layer F = 512 stack).
__global__ __launch_bounds__(256) void pack_conv_kernel(PackArgs p) {
  const int l = blockIdx.z, F = p.F;
  const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  __shared__ float t[3][32][33];                              // [tap][out - n0][in - c0]
  const float* w = p.w[l];
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r;
    for (int e = tx; e < 96; e += 32) {
      const int cl = e / 3, j = e - cl * 3;
      t[j][r][cl] = (n < F && c0 + cl < F) ? w[(long long)n * 3 * F + (long long)(c0 + cl) * 3 + j] : 0.f;
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, c = c0 + r;
    if (n < F && c0 + tx < F)
#pragma unroll
      for (int j = 0; j < 3; ++j) p.wf[l][(long long)n * 3 * F + j * F + c0 + tx] = t[j][r][tx];
    if (c < F && n0 + tx < F)
#pragma unroll
      for (int j = 0; j < 3; ++j) p.wb[l][(long long)c * 3 * F + j * F + n0 + tx] = t[j][tx][r];
  }
  if (p.wpt[l]) {
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int o = n0 + r;
      t[0][r][tx] = (o < F && c0 + tx < F) ? p.wpw[l][(long long)o * F + c0 + tx] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int c = c0 + r;
      if (c < F && n0 + tx < F) p.wpt[l][(long long)c * F + n0 + tx] = t[0][tx][r];
    }
  }
}

// ---- MS-TCN layout of saved activations / workspace --------------------------------
struct MstcnLayout {
  // every per-layer row slot holds rows_pad = rows rounded up to the 64-deep GEMM stage; the pad rows of
  // the h / z slots (forward) and of the deferred dZ / dH / dB slots (backward) are zero, so the deferred
  // weight-gradient GEMMs run over K = rows_pad on the FAST loaders (ragged batches included)
  long long rows_pad;
  long long rowsF;
  // saved
  long long h, z, xh, rs, wbs, wpts, wk1b, wk2b, total_saved;
  // workspace
  long long wf, wk1, wk2, buf0, buf1, buf2, buf3, buf4, buf5, split, split2, colsum, dzall, dhall, dball, csb, bsl,
      total_ws;
};

MstcnLayout mstcn_layout(const fx_mstcn_params* p, int rows) {
  MstcnLayout L{};
  const long long F = p->F;
  const int NL = p->num_layers;
  L.rows_pad = (long long)cdiv(rows, 64) * 64;
  L.rowsF = L.rows_pad * F;
  L.h = 0;                                   // h_0 .. h_NL
  L.z = L.h + (NL + 1) * L.rowsF;            // z_0 .. z_{NL-1}
  L.xh = L.z + NL * L.rowsF;                 // LN xhat_i
  L.rs = L.xh + (p->layernorm ? NL * L.rowsF : 0);
  L.wbs = L.rs + (p->layernorm ? (long long)NL * rows : 0);   // dX-packed conv weights (fwd packs, bwd reads)
  // grouped dilated convs (ngroup > 1): conv weight blocks of 3 F cg floats, no fused layers
  const int ng = mstcn_groups(p->ngroup, p->F);
  const bool fl = p->fused_layers && ng == 1;
  const long long wsz = 3 * F * (F / ng);
  L.wpts = L.wbs + NL * wsz;                 // transposed 1x1 weights (fwd packs, bwd dZ GEMM reads)
  L.wk1b = L.wpts + NL * F * F;              // fused layers: the backward chain's weights (the two above) in
  L.wk2b = L.wk1b + (fl ? NL * wsz : 0);     // MFMA fragment order, packed by the forward
  L.total_saved = L.wk2b + (fl ? NL * F * F : 0);
  L.wf = 0;
  L.wk1 = L.wf + NL * wsz;                   // fused layers: conv weights in MFMA fragment order
  L.wk2 = L.wk1 + (fl ? NL * wsz : 0);       // ... and the 1x1 weights
  L.buf0 = L.wk2 + (fl ? NL * F * F : 0);
  L.buf1 = L.buf0 + L.rowsF;
  L.buf2 = L.buf1 + L.rowsF;
  L.buf3 = L.buf2 + L.rowsF;                 // backward: third dH buffer, second dZ buffer (side stream)
  L.buf4 = L.buf3 + L.rowsF;
  L.buf5 = L.buf4 + L.rowsF;                 // third dZ buffer (fused backward chain)
  L.split = L.buf5 + L.rowsF;
  long long sp = 0;
  sp = std::max(sp, split_ws(p->F, 3 * p->F + 1, rows));      // conv dW (+ bias column)
  sp = std::max(sp, dwdb_ws(rows, p->F, p->F));               // pointwise dW
  sp = std::max(sp, split_ws(rows, p->F, p->F));              // pointwise dX (few rows: split K)
  sp = std::max(sp, dwdb_ws(rows, p->F, p->cout));            // out dW
  if (p->in_map) sp = std::max(sp, dwdb_ws(rows, p->cin, p->F));  // in dW
  sp = std::max(sp, split_ws(rows, p->F, p->cout));           // dH_L
  if (p->in_map) sp = std::max(sp, split_ws(rows, p->cin, p->F));
  sp = std::max(sp, layernorm_bwd_ws_floats(rows, p->F));
  if (ng > 1) sp = std::max(sp, gconv_dw_ws_floats(rows, p->F, ng));   // grouped conv dW partials
  L.split2 = L.split + sp;                   // split-K partials of the main stream's GEMMs
  L.colsum = L.split2 + sp;
  long long cs = colsum_workspace_floats(rows, std::max(std::max(p->F, p->cout), p->cin));
  // deferred weight gradients (fx_mstcn_bwd): every layer's dZ_i and dH_i+1 kept for the batched
  // dW GEMMs, and the batched conv-bias column sums
  L.dzall = L.colsum + cs;
  L.dhall = L.dzall + NL * L.rowsF;
  L.dball = L.dhall + NL * L.rowsF;          // training dropout: dB_i = dropout_i(dH_i+1), the 1x1 branch's gradient
  L.csb = L.dball + (p->dropout > 0.f ? NL * L.rowsF : 0);
  L.bsl = L.csb + (long long)NL * colsum_workspace_floats(rows, p->F);
  const int dsp = defer_split(rows);
  L.total_ws = L.bsl + std::max(split_ws(p->F, p->F + 1, rows, std::max(NL, 1)),
                                dsp > 1 ? (long long)dsp * std::max(NL, 1) * p->F * (3LL * p->F) : 0LL);
  return L;
}

// the fused layer kernel's weights: every layer's conv matrix (ld 3F) and 1x1 matrix (ld F) in fragment
// order, appended to a job list; the 1x1 sources are a per-layer pointer list or a base with a uniform
// stride
void frag_layer_jobs(std::vector<FragJob>& J, int NL, int F, const float* w1, long long w1_stride,
                     const float* const* w2list, const float* w2, long long w2_stride, float* dst1, float* dst2) {
  for (int l = 0; l < NL; ++l) {
    J.push_back({w1 + (long long)l * w1_stride, dst1 + (long long)l * frl_packed_floats(3 * F), 3 * F, 3 * F});
    J.push_back({w2list ? w2list[l] : w2 + (long long)l * w2_stride, dst2 + (long long)l * frl_packed_floats(F), F, F});
  }
}

int launch_frag_jobs(const std::vector<FragJob>& J, hipStream_t s) {
  for (size_t i = 0; i < J.size(); i += FRAG_JOBS)
    FX_TRY(launch_pack_frag(J.data() + i, (int)std::min<size_t>(FRAG_JOBS, J.size() - i), s));
  return FX_OK;
}

int layer_dilation(const fx_mstcn_params* p, int i) {
  long long d = p->dil0 > 0 ? p->dil0 : 1;
  const int f = p->dil_factor > 0 ? p->dil_factor : 2;
  for (int k = 0; k < i; ++k) d *= f;
  return (int)d;
}

// Whether the fused layer kernel (mstcn_fused.hip) serves this stack, `buf` being a buffer it would read.
// fx_mstcn_fwd asks with `saved`: true means every layer ran fused AND the forward packed the backward
// chain's fragment-order weights into `saved`.  fx_mstcn_bwd asks with its workspace for the fused chain.
bool mstcn_fused_ok(const fx_mstcn_params* p, const Seqs& q, const float* buf) {
  return p->fused_layers && p->ngroup <= 1 && !p->layernorm && frl_supported(p->F, buf, p->F, p->F) &&
         (!q.off || q.nvid <= 16) && (p->fused_layers == 2 || frl_fills_device(q.rows()));
}

// The batched weight-gradient GEMMs of fx_mstcn_bwd address layer i's gradients as layer 0's plus
// i times one stride: true for views of one flat gradient buffer in parameter order (FlatGradReducer).
// FX_MSTCN_DEFER=0 keeps the per-layer interleaved GEMMs (A/B).
bool mstcn_defer_ok(const fx_mstcn_params* p, const fx_mstcn_grads* g) {
  const int NL = p->num_layers;
  return knobs().mstcn_defer && uniform_stride(g->w_dil, NL) && uniform_stride(g->b_dil, NL) &&
         uniform_stride(g->w_pw, NL) && uniform_stride(g->b_pw, NL);
}

// ---- backward: the input-gradient chain dH_NL -> dH_0 runs on the caller's stream.  The weight-gradient GEMMs
// (dW_out, per layer dW_pw and the dilated-conv dW, dW_in) depend on the chain but nothing in the chain depends
// on them: they run on the side stream, overlapping the chain's GEMMs (each alone leaves the matrix pipes ~45 %
// idle in its prologue, barriers and epilogue).  Weight / bias gradients ACCUMULATE (+=) into g->* (the caller zeroes
// them once per step); every bias gradient rides in its weight-gradient GEMM (virtual ones column).  Four schedules:
enum class BwdSchedule {
  // Deferred (uniformly strided gradient buffers, no LayerNorm, dense convs, NL > 0): the chain keeps every
  // layer's dZ_i and dH_i+1 (with training dropout also the masked dB_i) in per-layer slots, and the weight
  // gradients of ALL layers follow it as batched GEMMs (batched_dw)
  FusedDeferred,   // ... and the fused layer kernel serves the stack: one kernel per layer of the chain
  GemmDeferred,    // ... and it does not: two GEMMs per layer
  // Not deferred: layer i's weight gradients run on the side stream while the chain computes layer i - 1;
  // the chain's buffers rotate (dH over 3, dZ over 2 or 3) and a main-stream write waits for the side
  // stream's layer that last read that buffer
  FusedPerLayer,   // the fused layer kernel serves the stack and there is no dropout
  PerLayer,        // everything else: LayerNorm or dropout (both single stream), grouped convs, zero layers
};

// what every schedule reads, filled once by fx_mstcn_bwd
struct MstcnBwd {
  const fx_mstcn_params* p;
  const fx_mstcn_grads* g;
  Seqs q;
  MstcnLayout L;
  const float* saved;
  float* ws;
  float* dx;         // the stack's input gradient (nullable), row stride lddx
  long long lddx;
  hipStream_t s;     // the chain's stream (= lane.main); lane.side: the weight gradients' stream
  SideLane lane;
  float *spl, *spm;  // split-K partials: the side stream's dW GEMMs / the main stream's GEMMs and LN backward
  const float *wk1, *wk2;   // fused chain: the dX-packed conv and transposed 1x1 weights in fragment order
  int rows, F, NL, ng;
  bool drop;
  float *Hb[3], *Zb[3];     // rotating dH / dZ buffers of the schedules that are not deferred
  const float* h(int i) const { return saved + L.h + i * L.rowsF; }
  const float* z(int i) const { return saved + L.z + i * L.rowsF; }
  // deferred slots: dZall(i) = dZ_i, dHall(i) = dH_i+1 (the gradient at layer i's output), dBall(i) = the 1x1
  // branch's gradient dropout_i(dH_i+1) with the forward's mask (basic.py:160), without dropout dH_i+1 itself
  float* dZall(int i) const { return ws + L.dzall + i * L.rowsF; }
  float* dHall(int i) const { return ws + L.dhall + i * L.rowsF; }
  float* dBall(int i) const { return drop ? ws + L.dball + i * L.rowsF : dHall(i); }
  int dil(int i) const { return layer_dilation(p, i); }
  int wait_side(int i) const { return i < NL ? lane.wait(i) : FX_OK; }   // main waits for the side stream's layer i
  int mask_dB(int i) const {
    if (!drop) return FX_OK;
    return launch_dropout(dHall(i), F, rows, F, F, 0, p->dropout, fx_drop_subseed(p->seed, i), dBall(i), F, s);
  }
  // dZ_i = (gB . W_pw,i) * (z_i > 0) with W_pw,i^T packed row-major by the forward: the B operand
  // loads as k-contiguous rows (b128 fragment reads) instead of the column-major weight
  int pw_dx(const float* gB, int i, float* dZ) const {
    fx_gemm_desc d = gemm_desc(rows, F, F, op_rows(gB, F), op_rows(saved + L.wpts + (long long)i * F * F, F), dZ, F);
    d.gate = z(i);
    d.ld_gate = F;
    d.split_k = pick_split(rows, F, F);
    d.workspace = spm;
    return launch_gemm(d, s);
  }
  // dW_pw,i += gB^T z_i, db_pw,i += colsum(gB)   (side)
  int pw_dw(const float* gB, int i) const {
    return linear_dwdb(gB, F, z(i), F, rows, F, F, g->w_pw[i], g->b_pw[i], 1, spl, lane.side);
  }
  // conv dW_i (tap-major columns stored straight into (F, F, 3)) + db_i (ones column)   (side)
  int conv_dw(int i, const float* dZi) const {
    if (ng > 1)   // one launch over every video and group, partials in the side stream's split region
      return launch_gconv_dw(dZi, F, h(i), F, rows, q.T, q.nvid, q.off, F, ng, dil(i), g->w_dil[i], g->b_dil[i], spl,
                             lane.side);
    return per_video(q, [&](int r0, int nr, const Seqs& qv) -> int {
      fx_operand b = conv_operand(h(i) + (long long)r0 * F, F, F, dil(i), 1, qv, true);
      b.ones_col = 3 * F + 1;
      fx_gemm_desc d = gemm_desc(F, 3 * F + 1, nr, op_cols(dZi + (long long)r0 * F, F), b, g->w_dil[i], 3 * F);
      d.c_tap_cin = F;
      d.c_last_col = g->b_dil[i];
      d.beta = 1.f;
      d.split_k = pick_split(F, 3 * F + 1, nr);
      d.workspace = spl;
      return launch_gemm(d, lane.side);
    });
  }
  // out = gU + conv_i^T(dZ) over the dX-packed weights of the forward
  int conv_dx(int i, const float* dZ, const float* gU, float* out, long long ldo) const {
    prof_begin(0, s);
    if (ng > 1) {
      FX_TRY(launch_gconv(dZ, F, rows, q.T, q.nvid, q.off, F, ng, dil(i), -1,
                          saved + L.wbs + i * gconv_packed_floats(F, ng), nullptr, 0, gU, F, 0, out, ldo, s));
    } else {
      fx_gemm_desc d = gemm_desc(rows, F, 3 * F, conv_operand(dZ, F, F, dil(i), -1, q, false),
                                 op_rows(saved + L.wbs + (long long)i * 3 * F * F, 3 * F), out, ldo);
      d.resid = gU;
      d.ld_resid = F;
      FX_TRY(launch_gemm(d, s));
    }
    prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (3.0 * rows * F + 3.0 * F * (F / ng)));
    return FX_OK;
  }
  // the fused layer step (mstcn_fused.hip), i >= 1: dH_i = gU + conv_i^T(dZ_i) and dZ_i-1 = (dH_i . W_pw,i-1) *
  // (z_i-1 > 0) in ONE kernel; with dBn the 1x1 product reads dB_i-1 = dropout_i-1(dH_i), also stored to dBn
  int frl_dx(int i, const float* dZi, const float* gU, float* dHi, float* dZn, float* dBn) const {
    return launch_frl(dZi, F, rows, q.T, dil(i), -1, q.off, q.nvid, wk1 + (long long)i * 3 * F * F, nullptr, 0, gU, F,
                      dHi, F, wk2 + (long long)(i - 1) * F * F, nullptr, nullptr, 0, z(i - 1), F, dZn, F, 0.f, 0, s,
                      dBn ? p->dropout : 0.f, dBn ? fx_drop_subseed(p->seed, i - 1) : 0, dBn, dBn ? F : 0);
  }
  // deferred schedules: dH_i = dH_i+1 + conv_i^T(dZ_i) into layer i - 1's slot.  The bottom layer's is the
  // stack's input gradient: straight into dx when there is no input map (*dH0 = nullptr), else Hb[0]
  int deferred_conv_dx(int i, const float** dH0) const {
    const bool to_dx = i == 0 && !p->in_map && dx;
    if (i == 0) *dH0 = to_dx ? nullptr : Hb[0];
    return conv_dx(i, dZall(i), dHall(i), i > 0 ? dHall(i - 1) : (to_dx ? dx : Hb[0]), to_dx ? lddx : F);
  }
  int batched_dw() const;
};

// Deferred schedules: the weight gradients of ALL layers, after the chain, as two batched GEMMs on the side
// stream -- the dilated-conv dW of every layer in one launch (per-layer dilation via b_dil_growth; NL x 24
// tiles of 128x64 over the full K = rows, no split-K slabs) and the 1x1 dW + db in another -- plus one batched
// column sum for the conv biases.  Per layer the interleaved version paid two split-K GEMMs and their reduce
// launches, competing with the chain for the CUs.  The slots' pad rows are zero: the GEMMs run over K = rows_pad.
int MstcnBwd::batched_dw() const {
  const int Kp = (int)L.rows_pad;
  WsBound wbb(ws + L.bsl, L.total_ws - L.bsl);
  FX_TRY(lane.fork(1));
  {   // 1x1: dW_pw,i += dB_i^T z_i, db_pw,i += colsum(dB_i)   (batched over layers)
    fx_operand b = op_cols(z(0), F);
    b.batch_stride = L.rowsF;
    b.ones_col = F + 1;
    fx_operand a = op_cols(dBall(0), F);
    a.batch_stride = L.rowsF;
    fx_gemm_desc d = gemm_desc(F, F + 1, Kp, a, b, g->w_pw[0], F);
    d.batch = NL;
    d.c_batch_stride = NL > 1 ? g->w_pw[1] - g->w_pw[0] : 0;
    d.c_last_col = g->b_pw[0];
    d.c_last_batch_stride = NL > 1 ? g->b_pw[1] - g->b_pw[0] : 0;
    d.beta = 1.f;
    d.split_k = std::max(pick_split(F, F + 1, rows, NL), defer_split(rows));
    d.workspace = ws + L.bsl;
    FX_TRY(launch_gemm(d, lane.side));
  }
  {   // dilated conv: dW_i += dZ_i^T taps(h_i) stored straight into (F, F, 3)   (batched over layers;
      // ragged videos in the same launch: the B loader finds each frame's video, gemm_dev.h COLS_CONVR)
    fx_operand b = conv_operand(h(0), F, F, dil(0), 1, q, true);
    b.batch_stride = L.rowsF;
    fx_operand a = op_cols(dZall(0), F);
    a.batch_stride = L.rowsF;
    fx_gemm_desc d = gemm_desc(F, 3 * F, Kp, a, b, g->w_dil[0], 3 * F);
    d.batch = NL;
    d.c_batch_stride = NL > 1 ? g->w_dil[1] - g->w_dil[0] : 0;
    d.b_dil_growth = p->dil_factor > 0 ? p->dil_factor : 2;
    d.c_tap_cin = F;
    d.beta = 1.f;
    d.split_k = defer_split(rows);
    d.workspace = ws + L.bsl;
    FX_TRY(launch_gemm(d, lane.side));
  }
  return launch_colsum_batched(dZall(0), F, L.rowsF, rows, F, NL, g->b_dil[0], NL > 1 ? g->b_dil[1] - g->b_dil[0] : 0,
                               1, ws + L.csb, lane.side);
}

// dZ_NL-1 by the 1x1 backward GEMM, then per layer ONE kernel for dH_i (-> dHall(i - 1)) and dZ_i-1
// (-> dZall(i - 1)), the bottom layer's conv backward alone, then every layer's weight gradients
int bwd_fused_deferred(const MstcnBwd& c, const float** dH0) {
  const int NL = c.NL, F = c.F, rows = c.rows;
  FX_TRY(c.mask_dB(NL - 1));
  FX_TRY(c.pw_dx(c.dBall(NL - 1), NL - 1, c.dZall(NL - 1)));
  if (NL > 1) prof_begin(7, c.s);   // (the chain of NL - 1 back-to-back launches timed as one)
  for (int i = NL - 1; i >= 1; --i)
    FX_TRY(c.frl_dx(i, c.dZall(i), c.dHall(i), c.dHall(i - 1), c.dZall(i - 1), c.drop ? c.dBall(i - 1) : nullptr));
  if (NL > 1)
    prof_end(7, c.s, (NL - 1) * 2.0 * rows * F * 4.0 * F, (NL - 1) * 4.0 * (4.0 * rows * F + 4.0 * F * F), NL - 1);
  FX_TRY(c.deferred_conv_dx(0, dH0));
  return c.batched_dw();
}

// per layer dB_i (dropout), dZ_i by the 1x1 backward GEMM, dH_i by the conv backward GEMM; then every layer's dW
int bwd_gemm_deferred(const MstcnBwd& c, const float** dH0) {
  for (int i = c.NL - 1; i >= 0; --i) {
    FX_TRY(c.mask_dB(i));
    FX_TRY(c.pw_dx(c.dBall(i), i, c.dZall(i)));
    FX_TRY(c.deferred_conv_dx(i, dH0));
  }
  return c.batched_dw();
}

// dH_i lives in Hb[(NL - i) % 3], dZ_i in Zb[(NL - 1 - i) % 3]; a kernel overwriting a buffer first waits
// for the side stream's layer that last read it (layer i + 2 for both)
int bwd_fused_per_layer(const MstcnBwd& c, const float** dH0) {
  const int NL = c.NL, F = c.F, rows = c.rows;
  const int top = NL - 1;   // top layer: dZ by the 1x1 backward GEMM
  FX_TRY(c.lane.fork(1));
  FX_TRY(c.pw_dw(c.Hb[0], top));
  FX_TRY(linear_dx(c.Hb[0], F, c.p->w_pw[top], rows, F, F, c.Zb[0], F, 0, c.z(top), F, c.spm, c.s));
  FX_TRY(c.lane.fork(2));
  FX_TRY(c.conv_dw(top, c.Zb[0]));
  FX_TRY(c.lane.done(top));
  for (int i = NL - 1; i >= 0; --i) {
    const float* gU = c.Hb[(NL - 1 - i) % 3];   // dH_{i+1}
    const float* dZi = c.Zb[(NL - 1 - i) % 3];
    float* dHi = c.Hb[(NL - i) % 3];
    FX_TRY(c.wait_side(i + 2));
    if (i == 0) {   // the bottom layer: conv backward only
      FX_TRY(c.conv_dx(0, dZi, gU, dHi, F));
    } else {
      float* dZn = c.Zb[(NL - i) % 3];
      prof_begin(7, c.s);
      FX_TRY(c.frl_dx(i, dZi, gU, dHi, dZn, nullptr));
      prof_end(7, c.s, 2.0 * rows * F * 4.0 * F, 4.0 * (4.0 * rows * F + 4.0 * F * F));
      FX_TRY(c.lane.fork(1));
      FX_TRY(c.pw_dw(dHi, i - 1));
      FX_TRY(c.conv_dw(i - 1, dZn));
      FX_TRY(c.lane.done(i - 1));
    }
    *dH0 = dHi;
  }
  return FX_OK;
}

// per layer: [LayerNorm backward,] [dropout mask,] 1x1 dW (side) and dZ (main), conv dW (side) and dH (main).
// With a side stream (no LayerNorm, no dropout) dZ alternates over Zb[0 / 1] and dH rotates over Hb.
int bwd_per_layer(const MstcnBwd& c, const float** dH0) {
  const fx_mstcn_params* p = c.p;
  const int NL = c.NL, F = c.F, rows = c.rows;
  float* dH = c.Hb[0];
  float* dU = c.ws + c.L.buf1;   // LayerNorm: gradient at the residual sum (pre-LN)
  for (int i = NL - 1; i >= 0; --i) {
    const int step = NL - 1 - i;
    const float* gU = dH;
    if (p->layernorm) {
      FX_TRY(launch_layernorm_bwd(dH, F, nullptr, 0, c.saved + c.L.xh + i * c.L.rowsF, F, p->ln_w[i],
                                  c.saved + c.L.rs + (long long)i * rows, rows, F, 0, dU, F, c.g->ln_w[i],
                                  c.g->ln_b[i], c.spm, c.s));
      gU = dU;
    }
    // the 1x1 branch saw dropout: its gradient is gU masked the same way (the residual keeps gU)
    const float* gB = gU;
    if (c.drop) {
      float* gm = c.ws + c.L.buf4;   // (single stream: dZ stays in buf2, buf4 is free)
      FX_TRY(launch_dropout(gU, F, rows, F, F, 0, p->dropout, fx_drop_subseed(p->seed, i), gm, F, c.s));
      gB = gm;
    }
    FX_TRY(c.lane.fork(1));
    FX_TRY(c.pw_dw(gB, i));
    float* dZ = c.lane.ss ? c.Zb[step & 1] : c.Zb[0];
    FX_TRY(c.wait_side(i + 2));   // dZ buffer last read by layer i + 2's conv dW
    FX_TRY(c.pw_dx(gB, i, dZ));
    FX_TRY(c.lane.fork(2));
    FX_TRY(c.conv_dw(i, dZ));
    FX_TRY(c.lane.done(i));
    // dH_i = gU + conv^T(dZ).  LayerNorm: gU is dU, and dH_i overwrites dH_i+1 in place
    float* dHn = p->layernorm ? dH : c.Hb[(step + 1) % 3];
    if (!p->layernorm) FX_TRY(c.wait_side(i + 2));   // that buffer was gU of layer i + 2
    FX_TRY(c.conv_dx(i, dZ, gU, dHn, F));
    dH = dHn;
  }
  *dH0 = dH;
  return FX_OK;
}

}  // namespace

int pack_conv_set(const float* const* w, int NL, int F, int ng, float* wf, float* wb, const float* const* wpw,
                  float* wpt, hipStream_t s) {
  if (ng > 1) {   // grouped: per-group tap-major images (conv_grouped.hip)
    const long long gsz = gconv_packed_floats(F, ng);
    std::vector<GPackJob> J;
    for (int l = 0; l < NL; ++l)
      J.push_back({w[l], wf + l * gsz, wb + l * gsz, wpw ? wpw[l] : nullptr, wpt ? wpt + (long long)l * F * F : nullptr});
    return J.empty() ? FX_OK : launch_gconv_pack(J.data(), NL, F, ng, s);
  }
  PackArgs a{};
  a.F = F;
  const long long wsz = 3LL * F * F;
  for (int l = 0; l < NL; ++l) {
    a.w[l] = w[l];
    a.wf[l] = wf + l * wsz;
    a.wb[l] = wb + l * wsz;
    a.wpw[l] = wpw ? wpw[l] : nullptr;
    a.wpt[l] = wpt ? wpt + (long long)l * F * F : nullptr;
  }
  fx_launch(pack_conv_kernel, dim3(cdiv(F, 32), cdiv(F, 32), NL), dim3(256), 0, s, a);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx

using namespace fx;

extern "C" {

// ---------------------------------------------------------------- MS-TCN
long long fx_mstcn_saved_floats(const fx_mstcn_params* p, int rows) { return mstcn_layout(p, rows).total_saved; }
long long fx_mstcn_workspace_floats(const fx_mstcn_params* p, int rows) { return mstcn_layout(p, rows).total_ws; }

int fx_mstcn_fwd(const fx_mstcn_params* p, const float* x, long long ldx, int T, int nvid, float* y, long long ldy,
                 float* saved, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(p && p->num_layers >= 0 && p->num_layers <= 32, "mstcn: 0..32 layers");
  FX_REQUIRE(p->in_map || p->cin == p->F, "mstcn: in_map=0 needs cin == F");
  FX_TRY(gconv_check(p->F, p->ngroup, "mstcn"));
  const Seqs q{T, nvid, p->seq_off};
  FX_TRY(check_seqs(q));
  const int rows = q.rows();
  const int F = p->F;
  const int ng = mstcn_groups(p->ngroup, F);
  const MstcnLayout L = mstcn_layout(p, rows);
  FX_TRY(pack_conv_set(p->w_dil, p->num_layers, F, ng, workspace + L.wf, saved + L.wbs, p->w_pw, saved + L.wpts, s));
  if (L.rows_pad > rows && p->num_layers > 0)   // pad rows of h_0 .. h_NL, z_0 .. z_NL-1 (adjacent slots)
    FX_CHECK_HIP(hipMemset2DAsync(saved + L.h + (long long)rows * F, L.rowsF * sizeof(float), 0,
                                  (L.rows_pad - rows) * F * sizeof(float), 2 * p->num_layers + 1, s));
  float* h0 = saved + L.h;
  if (p->in_map) {
    FX_TRY(linear_fwd(x, ldx, rows, p->cin, p->w_in, p->b_in, h0, F, F, 0, s));
  } else {
    FX_CHECK_HIP(hipMemcpy2DAsync(h0, F * sizeof(float), x, ldx * sizeof(float), F * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, s));
  }
  const bool fused = mstcn_fused_ok(p, q, saved);
  if (fused && p->num_layers > 0) {
    // one launch: this pass's weights (conv from the pack above, 1x1 as given) and the backward chain's
    // (the dX-packed conv and transposed 1x1 weights packed above into `saved`), so the backward packs none
    std::vector<FragJob> J;
    frag_layer_jobs(J, p->num_layers, F, workspace + L.wf, 3LL * F * F, p->w_pw, nullptr, 0, workspace + L.wk1,
                    workspace + L.wk2);
    frag_layer_jobs(J, p->num_layers, F, saved + L.wbs, 3LL * F * F, nullptr, saved + L.wpts, (long long)F * F,
                    saved + L.wk1b, saved + L.wk2b);
    FX_TRY(launch_frag_jobs(J, s));
  }
  for (int i = 0; i < p->num_layers; ++i) {
    const float* hi = saved + L.h + i * L.rowsF;
    float* hn = saved + L.h + (i + 1) * L.rowsF;
    float* zi = saved + L.z + i * L.rowsF;
    if (fused) {   // z = relu(conv(h) + b); h' = h + dropout(z . Wpw^T + b): one kernel (mstcn_fused.hip)
      // (timed as one chain: an event pair around every launch would add its own dispatch gap)
      if (i == 0) prof_begin(7, s);
      FX_TRY(launch_frl(hi, F, rows, T, layer_dilation(p, i), 1, q.off, q.nvid,
                        workspace + L.wk1 + (long long)i * 3 * F * F, p->b_dil[i], 1, nullptr, 0, zi, F,
                        workspace + L.wk2 + (long long)i * F * F, p->b_pw[i], hi, F, nullptr, 0, hn, F, p->dropout,
                        fx_drop_subseed(p->seed, i), s));
      if (i == p->num_layers - 1)
        prof_end(7, s, p->num_layers * 2.0 * rows * F * 4.0 * F, p->num_layers * 4.0 * (3.0 * rows * F + 4.0 * F * F),
                 p->num_layers);
      continue;
    }
    // z = relu(dilated_conv(h) + b)      (basic.py:158)
    if (ng > 1) {   // grouped conv kernel: K = 3 F / ng per output column
      prof_begin(0, s);
      FX_TRY(launch_gconv(hi, F, rows, T, q.nvid, q.off, F, ng, layer_dilation(p, i), 1,
                          workspace + L.wf + i * gconv_packed_floats(F, ng), p->b_dil[i], 1, nullptr, 0, 0, zi, F, s));
      prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (2.0 * rows * F + 3.0 * F * (F / ng)));
    } else {
      fx_gemm_desc d = gemm_desc(rows, F, 3 * F, conv_operand(hi, F, F, layer_dilation(p, i), 1, q, false),
                                 op_rows(workspace + L.wf + (long long)i * 3 * F * F, 3 * F), zi, F);
      d.bias = p->b_dil[i];
      d.relu = 1;
      prof_begin(0, s);
      FX_TRY(launch_gemm(d, s));
      prof_end(0, s, 2.0 * rows * F * 3.0 * F, 4.0 * (2.0 * rows * F + 3.0 * F * F));
    }
    // h' = h + z . Wpw^T + b   [then LN]   (basic.py:159-169)
    float* u = p->layernorm ? workspace + L.buf0 : hn;
    fx_gemm_desc e = gemm_desc(rows, F, F, op_rows(zi, F), op_rows(p->w_pw[i], F), u, F);
    e.bias = p->b_pw[i];
    e.resid = hi;
    e.ld_resid = F;
    e.drop_p = p->dropout;   // h' = h + dropout(z . Wpw^T + b)   (basic.py:160)
    e.drop_seed = fx_drop_subseed(p->seed, i);
    FX_TRY(launch_gemm(e, s));
    if (p->layernorm)
      FX_TRY(launch_layernorm_fwd(u, F, nullptr, 0, p->ln_w[i], p->ln_b[i], 1e-5f, rows, F, 0, hn, F, nullptr,
                                  saved + L.rs + (long long)i * rows, saved + L.xh + i * L.rowsF, F, s));
  }
  const float* hL = saved + L.h + p->num_layers * L.rowsF;
  return linear_fwd(hL, F, rows, F, p->w_out, p->b_out, y, ldy, p->cout, 0, s);
}

int fx_mstcn_bwd(const fx_mstcn_params* p, const fx_mstcn_grads* g, const float* x, long long ldx, int T, int nvid,
                 const float* dy, long long lddy, float* dx, long long lddx, const float* saved, float* ws,
                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const Seqs q{T, nvid, p->seq_off};
  FX_TRY(check_seqs(q));
  const int rows = q.rows(), F = p->F, NL = p->num_layers;
  const MstcnLayout L = mstcn_layout(p, rows);
  FX_REQUIRE(p->dropout >= 0.f && p->dropout < 1.f, "mstcn: dropout must be in [0, 1)");
  FX_TRY(gconv_check(F, p->ngroup, "mstcn"));
  const int ng = mstcn_groups(p->ngroup, F);
  const bool drop = p->dropout > 0.f;
  // Which schedule.  (Deferred even for the input block's stack, the LAST work of the backward pass, whose batched
  // dW runs after the chain with nothing left to overlap, a ~0.7 ms side-stream tail: the per-layer schedule there,
  // or the upper layers' dW mid-chain, measured even -- the overlapped GEMMs slow the chain as much, rounds 3 and 5)
  const bool defer = !p->layernorm && NL > 0 && ng == 1 && mstcn_defer_ok(p, g);
  const bool drop_chain_ok = !drop || defer;   // the fused chain masks dB only into the deferred slots
  const bool fchain = NL > 0 && drop_chain_ok && mstcn_fused_ok(p, q, ws + L.buf0);
  const BwdSchedule sched = fchain ? (defer ? BwdSchedule::FusedDeferred : BwdSchedule::FusedPerLayer)
                                   : (defer ? BwdSchedule::GemmDeferred : BwdSchedule::PerLayer);
  // (LayerNorm, and dropout without deferral: single stream)
  MstcnBwd c{p, g, q, L, saved, ws, dx, lddx, s, side_lane(s, !p->layernorm && drop_chain_ok), ws + L.split,
             ws + L.split2, saved + L.wk1b, saved + L.wk2b, rows, F, NL, ng, drop,
             {ws + L.buf0, ws + L.buf1, ws + L.buf3}, {ws + L.buf2, ws + L.buf4, ws + L.buf5}};
  // the fused chain's fragment-order weights: packed by a fused forward into `saved`, else here from the
  // forward's dX-packed conv weights and transposed 1x1 weights
  if (fchain && !mstcn_fused_ok(p, q, saved)) {
    std::vector<FragJob> J;
    frag_layer_jobs(J, NL, F, saved + L.wbs, 3LL * F * F, nullptr, saved + L.wpts, (long long)F * F, ws + L.wk1,
                    ws + L.wk2);
    FX_TRY(launch_frag_jobs(J, s));
    c.wk1 = ws + L.wk1;
    c.wk2 = ws + L.wk2;
  }
  WsBound wb(c.spl, L.colsum - L.split);
  // deferred: the pad rows of the dZ / dH (/ dB) slots are zero, so the batched dW GEMMs run over K = rows_pad
  if (defer && L.rows_pad > rows)
    FX_CHECK_HIP(hipMemset2DAsync(ws + L.dzall + (long long)rows * F, L.rowsF * sizeof(float), 0,
                                  (L.rows_pad - rows) * F * sizeof(float), (drop ? 3 : 2) * NL, s));
  // prologue: dW_out, db_out (side) and dH_NL = dy . W_out (deferred: kept in its slot for the 1x1 dW)
  FX_TRY(c.lane.fork(0));
  FX_TRY(linear_dwdb(dy, lddy, c.h(NL), F, rows, F, p->cout, g->w_out, g->b_out, 1, c.spl, c.lane.side));
  float* dHtop = defer ? c.dHall(NL - 1) : c.Hb[0];
  FX_TRY(linear_dx(dy, lddy, p->w_out, rows, F, p->cout, dHtop, F, 0, nullptr, 0, c.spm, s));
  const float* dH = c.Hb[0];   // dH_0 after the chain (nullptr: already in dx)
  switch (sched) {
    case BwdSchedule::FusedDeferred: FX_TRY(bwd_fused_deferred(c, &dH)); break;
    case BwdSchedule::GemmDeferred: FX_TRY(bwd_gemm_deferred(c, &dH)); break;
    case BwdSchedule::FusedPerLayer: FX_TRY(bwd_fused_per_layer(c, &dH)); break;
    case BwdSchedule::PerLayer: FX_TRY(bwd_per_layer(c, &dH)); break;
  }
  // epilogue: the input map's gradients, or dH_0 copied to dx; join
  if (p->in_map) {
    if (g->w_in) {
      FX_TRY(c.lane.fork(0));
      FX_TRY(linear_dwdb(dH, F, x, ldx, rows, p->cin, F, g->w_in, g->b_in, 1, c.spl, c.lane.side));
    }
    if (dx) FX_TRY(linear_dx(dH, F, p->w_in, rows, p->cin, F, dx, lddx, 0, nullptr, 0, c.spm, s));
  } else if (dx && dH) {
    FX_CHECK_HIP(hipMemcpy2DAsync(dx, lddx * sizeof(float), dH, F * sizeof(float), F * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, s));
  }
  return c.lane.join(p->side_defer);   // everything the side stream did is ordered before later work
}

}  // extern "C"
