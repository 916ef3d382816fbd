// MS-TCN++ (MSTCN2) stack and the single grouped dilated conv layer.
#include <algorithm>
#include <vector>

#include "fx_common.h"
#include "ops.h"
#include "frames.h"

namespace fx {
namespace {

struct Mstcn2Layout {
  long long rowsF;
  long long f, cat, r, wb1, wb2, total_saved;            // saved: f_0..f_L, cat_i (2F), r_i, dX-packed weights
  long long wf1, wf2, hb0, hb1, du, dcat, spm, spl, bsl, wk, total_ws;
};

// the fused layer kernel (mstcn2_fused.hip) can serve stacks of this shape: what the size functions reserve for
// (whether a call takes it also depends on its rows, videos, buffers and stream: mstcn2_fused_ok)
bool mstcn2_fused_shape(const fx_mstcn2_params* p) { return p->fused_layers && p->F == 256 && p->ngroup <= 1; }
// fragment-order weights of one fused pass: per layer two conv matrices (3 F F each) and the fusion matrix (2 F F)
long long mstcn2_frag_floats(int F) { return 2 * frl_packed_floats(3 * F) + frl_packed_floats(2 * F); }

Mstcn2Layout mstcn2_layout(const fx_mstcn2_params* p, int rows) {
  Mstcn2Layout L{};
  const long long F = p->F;
  const int NL = p->num_layers;
  L.rowsF = (long long)rows * F;
  L.f = 0;
  L.cat = L.f + (NL + 1) * L.rowsF;
  L.r = L.cat + 2 * NL * L.rowsF;
  const int ng = mstcn_groups(p->ngroup, p->F);
  const long long wsz = 3 * F * (F / ng);   // (grouped dilated convs: 3 F cg per conv)
  L.wb1 = L.r + NL * L.rowsF;
  L.wb2 = L.wb1 + NL * wsz;
  L.total_saved = L.wb2 + NL * wsz;
  L.wf1 = 0;
  L.wf2 = L.wf1 + NL * wsz;
  L.hb0 = L.wf2 + NL * wsz;                 // input-gradient chain: dF ping-pong
  L.hb1 = L.hb0 + L.rowsF;
  L.du = L.hb1 + L.rowsF;                   // every layer's dU_i (fusion pre-activation gradient)
  L.dcat = L.du + NL * L.rowsF;             // every layer's dCat_i = [dA_i | dB_i]
  L.spm = L.dcat + 2 * NL * L.rowsF;        // split-K partials: main-stream GEMMs
  long long sp = 0;
  sp = std::max(sp, split_ws(rows, F, p->cout));
  sp = std::max(sp, split_ws(rows, 2 * F, F));
  sp = std::max(sp, split_ws(rows, F, 3 * F));
  if (p->in_map) sp = std::max(sp, split_ws(rows, p->cin, F));
  L.spl = L.spm + sp;                       // ... side stream (out / in map dW)
  long long sl = std::max(dwdb_ws(rows, F, p->cout), p->in_map ? dwdb_ws(rows, p->cin, F) : 0LL);
  L.bsl = L.spl + sl;                       // ... the (batched) layer dW GEMMs
  long long sb = 0;
  for (int nb : {1, std::max(NL, 1)}) {
    sb = std::max(sb, split_ws(F, 2 * F + 1, rows, nb));
    sb = std::max(sb, split_ws(F, 3 * F + 1, rows, nb));
  }
  if (ng > 1) sb = std::max(sb, gconv_dw_ws_floats(rows, p->F, ng));   // grouped conv dW partials
  // fused layers: this pass's weights in MFMA fragment order (the forward's three matrices per layer, or the
  // backward chain's -- each call packs its own, so a backward never depends on what the forward ran)
  L.wk = al64(L.bsl + sb);
  L.total_ws = mstcn2_fused_shape(p) ? L.wk + NL * mstcn2_frag_floats(p->F) : L.bsl + sb;
  return L;
}

int mstcn2_dil(const fx_mstcn2_params* p, int e) {   // dil_factor^e
  const int f = p->dil_factor > 0 ? p->dil_factor : 2;
  long long d = 1;
  for (int k = 0; k < e; ++k) d *= f;
  return (int)d;
}

// Whether the fused layer kernel serves this call, `buf` being the buffer of row slots it would read.
// fx_mstcn2_fwd and fx_mstcn2_bwd each ask for themselves.  The bf16 / split precision modes exist for their
// arithmetic: a stream in one of them keeps its GEMM kernels.
bool mstcn2_fused_ok(const fx_mstcn2_params* p, const Seqs& q, const float* buf, hipStream_t s) {
  return mstcn2_fused_shape(p) && frl_supported(p->F, buf, p->F, 2 * p->F) && (!q.off || q.nvid <= 16) &&
         fx_get_stream_precision(s) == FX_PREC_F32 &&
         (p->fused_layers == 2 || frl_fills_device(q.rows(), knobs().frl2_min_fill));
}

constexpr int kProfFrl2 = 15;   // fx_prof kind of the fused MS-TCN++ layer chains

}  // namespace
}  // namespace fx

using namespace fx;

extern "C" {

long long fx_mstcn2_saved_floats(const fx_mstcn2_params* p, int rows) { return mstcn2_layout(p, rows).total_saved; }
long long fx_mstcn2_workspace_floats(const fx_mstcn2_params* p, int rows) { return mstcn2_layout(p, rows).total_ws; }

int fx_mstcn2_fwd(const fx_mstcn2_params* p, const float* x, long long ldx, int T, int nvid, float* y, long long ldy,
                  float* saved, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(p && p->num_layers >= 0 && p->num_layers <= 32, "mstcn2: 0..32 layers");
  FX_REQUIRE(p->in_map || p->cin == p->F, "mstcn2: in_map=0 needs cin == F");
  FX_REQUIRE(p->dropout >= 0.f && p->dropout < 1.f, "mstcn2: dropout must be in [0, 1)");
  FX_REQUIRE(saved && workspace && y, "mstcn2: bad arguments");
  FX_TRY(gconv_check(p->F, p->ngroup, "mstcn2"));
  const Seqs q{T, nvid, p->seq_off};
  FX_TRY(check_seqs(q));
  const int rows = q.rows(), F = p->F, NL = p->num_layers;
  const int ng = mstcn_groups(p->ngroup, F);
  const long long gsz = gconv_packed_floats(F, ng);
  const Mstcn2Layout L = mstcn2_layout(p, rows);
  float* ws = workspace;
  if (NL > 0) {   // forward images into the workspace, dX images into `saved` for the backward
    FX_TRY(pack_conv_set(p->w_d1, NL, F, ng, ws + L.wf1, saved + L.wb1, nullptr, nullptr, s));
    FX_TRY(pack_conv_set(p->w_d2, NL, F, ng, ws + L.wf2, saved + L.wb2, nullptr, nullptr, s));
  }
  float* f0 = saved + L.f;
  if (p->in_map) {
    FX_TRY(linear_fwd(x, ldx, rows, p->cin, p->w_in, p->b_in, f0, F, F, 0, s));
  } else {
    FX_CHECK_HIP(hipMemcpy2DAsync(f0, F * sizeof(float), x, ldx * sizeof(float), F * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, s));
  }
  const bool fused = NL > 0 && mstcn2_fused_ok(p, q, saved, s) && frl_supported(F, ws + L.wk, F, F);
  if (fused) {   // the conv images packed above and W_fu as given, in fragment order: one pack launch
    const long long c3 = frl_packed_floats(3 * F), per = mstcn2_frag_floats(F);
    std::vector<FragJob> J;
    for (int i = 0; i < NL; ++i) {
      float* wk = ws + L.wk + i * per;
      J.push_back({ws + L.wf1 + i * c3, wk, 3 * F, 3 * F});
      J.push_back({ws + L.wf2 + i * c3, wk + c3, 3 * F, 3 * F});
      J.push_back({p->w_fu[i], wk + 2 * c3, 2 * F, 2 * F});
    }
    for (size_t j = 0; j < J.size(); j += FRAG_JOBS)
      FX_TRY(launch_pack_frag(J.data() + j, (int)std::min<size_t>(FRAG_JOBS, J.size() - j), s));
    // cat_i, r_i and f_i+1 of every layer: one kernel per layer (timed as one chain, like kind 7)
    prof_begin(kProfFrl2, s);
    for (int i = 0; i < NL; ++i) {
      const float* wk = ws + L.wk + i * per;
      const Frl2Layer y{rows, T, mstcn2_dil(p, NL - 1 - i), mstcn2_dil(p, i), q.off, q.nvid,
                        i != NL - 1 ? p->dropout : 0.f, fx_drop_subseed(p->seed, i)};
      FX_TRY(launch_frl2_fwd(y, saved + L.f + i * L.rowsF, wk, wk + c3, p->b_d1[i], p->b_d2[i],
                             saved + L.cat + 2 * i * L.rowsF, wk + 2 * c3, p->b_fu[i], saved + L.r + i * L.rowsF,
                             saved + L.f + (i + 1) * L.rowsF, s));
    }
    prof_end(kProfFrl2, s, NL * 2.0 * rows * F * 8.0 * F, NL * 4.0 * (5.0 * rows * F + 8.0 * F * F), NL);
  }
  for (int i = 0; i < NL && !fused; ++i) {
    const float* fi = saved + L.f + i * L.rowsF;
    float* fn = saved + L.f + (i + 1) * L.rowsF;
    float* cat = saved + L.cat + 2 * i * L.rowsF;
    float* ri = saved + L.r + i * L.rowsF;
    // cat = [conv_d1(f) | conv_d2(f)]: the two dilated convs store into the halves of one buffer
    // (no torch.cat)   (basic.py:276)
    // (one batch-2 launch: batch h takes conv h's dilation, packed weights, bias and output half --
    // at Breakfast's 2048 rows the pair fills the chip with 128x64 tiles where one conv could not)
    if (ng > 1) {   // grouped: one grouped-conv launch per dilated conv, each into its half of cat
      for (int h = 0; h < 2; ++h) {
        prof_begin(0, s);
        FX_TRY(launch_gconv(fi, F, rows, T, q.nvid, q.off, F, ng, mstcn2_dil(p, h == 0 ? NL - 1 - i : i), 1,
                            ws + (h == 0 ? L.wf1 : L.wf2) + i * gsz, h == 0 ? p->b_d1[i] : p->b_d2[i], 0, nullptr, 0,
                            0, cat + h * F, 2 * F, s));
        prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (2.0 * rows * F + 3.0 * F * (F / ng)));
      }
    } else {
      fx_gemm_desc d = gemm_desc(rows, F, 3 * F, conv_operand(fi, F, F, mstcn2_dil(p, NL - 1 - i), 1, q, false),
                                 op_rows(ws + L.wf1 + (long long)i * 3 * F * F, 3 * F), cat, 2 * F);
      d.batch = 2;
      d.a_dil_b1 = mstcn2_dil(p, i);
      d.b.batch_stride = L.wf2 - L.wf1;
      d.c_batch_stride = F;
      d.bias = p->b_d1[i];
      d.bias_batch_stride = p->b_d2[i] - p->b_d1[i];
      prof_begin(0, s);
      FX_TRY(launch_gemm(d, s));
      prof_end(0, s, 2.0 * 2.0 * rows * F * 3.0 * F, 4.0 * (3.0 * rows * F + 6.0 * F * F));
    }
    // r = dropout(relu(W_fu . cat + b_fu)) (no dropout on the last layer), f' = f + r  (basic.py:276-280)
    fx_gemm_desc e = gemm_desc(rows, F, 2 * F, op_rows(cat, 2 * F), op_rows(p->w_fu[i], 2 * F), ri, F);
    e.bias = p->b_fu[i];
    e.relu = 2;
    if (i != NL - 1) {
      e.drop_p = p->dropout;
      e.drop_seed = fx_drop_subseed(p->seed, i);
    }
    FX_TRY(launch_gemm(e, s));
    FX_TRY(add2(fi, F, ri, F, rows, F, fn, F, 0, s));
  }
  return linear_fwd(saved + L.f + NL * L.rowsF, F, rows, F, p->w_out, p->b_out, y, ldy, p->cout, 0, s);
}

int fx_mstcn2_bwd(const fx_mstcn2_params* p, const fx_mstcn2_grads* g, const float* x, long long ldx, int T, int nvid,
                  const float* dy, long long lddy, float* dx, long long lddx, const float* saved, float* workspace,
                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_REQUIRE(p && g && saved && workspace && dy, "mstcn2 bwd: bad arguments");
  FX_TRY(gconv_check(p->F, p->ngroup, "mstcn2"));
  const Seqs q{T, nvid, p->seq_off};
  FX_TRY(check_seqs(q));
  const int rows = q.rows(), F = p->F, NL = p->num_layers;
  const int ng = mstcn_groups(p->ngroup, F);
  const long long gsz = gconv_packed_floats(F, ng);
  const Mstcn2Layout L = mstcn2_layout(p, rows);
  float* ws = workspace;
  const SideLane lane = side_lane(s);   // weight gradients on the side stream
  const hipStream_t sd = lane.side;
  float* spm = ws + L.spm;
  float* spl = ws + L.spl;
  const float* fL = saved + L.f + NL * L.rowsF;
  FX_TRY(lane.fork(0));
  {
    WsBound wb(spl, L.bsl - L.spl);
    FX_TRY(linear_dwdb(dy, lddy, fL, F, rows, F, p->cout, g->w_out, g->b_out, 1, spl, sd));
  }
  WsBound wbm(spm, L.spl - L.spm);
  float* Hb[2] = {ws + L.hb0, ws + L.hb1};
  float* gF = Hb[0];
  FX_TRY(linear_dx(dy, lddy, p->w_out, rows, F, p->cout, gF, F, 0, nullptr, 0, spm, s));
  // Fused chain (mstcn2_fused.hip): the top layer's dU / dCat and the bottom layer's two conv GEMMs stay as
  // below; in between, ONE kernel per layer forms G_i, dU_i-1 and dCat_i-1.  Its fragment-order weights are
  // packed here from the forward's dX images in `saved` and from W_fu, whatever path the forward took.
  const bool fchain = NL > 1 && mstcn2_fused_ok(p, q, ws + L.hb0, s) && frl_supported(F, ws + L.wk, F, F);
  const long long c3 = frl_packed_floats(3 * F), per = mstcn2_frag_floats(F);
  if (fchain) {
    std::vector<FragJob> J;
    for (int i = 0; i < NL; ++i) {
      float* wk = ws + L.wk + i * per;
      if (i >= 1) {   // conv^T of layers L-1 .. 1
        J.push_back({saved + L.wb1 + i * c3, wk, 3 * F, 3 * F});
        J.push_back({saved + L.wb2 + i * c3, wk + c3, 3 * F, 3 * F});
      }
      if (i < NL - 1)   // the halves of W_fu^T of layers L-2 .. 0
        for (int h = 0; h < 2; ++h) J.push_back({p->w_fu[i] + h * F, wk + 2 * c3 + (long long)h * F * F, 2 * F, F, 1});
    }
    for (size_t j = 0; j < J.size(); j += FRAG_JOBS)
      FX_TRY(launch_pack_frag(J.data() + j, (int)std::min<size_t>(FRAG_JOBS, J.size() - j), s));
  }
  for (int i = NL - 1; i >= 0; --i) {
    const float* ri = saved + L.r + i * L.rowsF;
    float* dU = ws + L.du + i * L.rowsF;
    float* dCat = ws + L.dcat + 2 * i * L.rowsF;
    float* dFn = Hb[(NL - i) & 1];
    if (!(fchain && i < NL - 1)) {   // (fused chain: layer i + 1's step left dU_i and dCat_i in their slots)
      // dU = dropout_i(gF) * (r_i > 0)   (r_i is stored after the dropout: zero where dropped)
      if (i != NL - 1 && p->dropout > 0.f) {
        FX_TRY(launch_dropout(gF, F, rows, F, F, 0, p->dropout, fx_drop_subseed(p->seed, i), dU, F, s));
        FX_TRY(relu_bwd(dU, F, ri, F, rows, F, dU, F, s));
      } else {
        FX_TRY(relu_bwd(gF, F, ri, F, rows, F, dU, F, s));
      }
      // dCat = dU . W_fu   (rows x 2F)
      FX_TRY(launch_gemm(gemm_desc(rows, 2 * F, F, op_rows(dU, F), op_cols(p->w_fu[i], 2 * F), dCat, 2 * F), s));
    }
    if (fchain && i >= 1) {   // G_i, dU_i-1 and dCat_i-1 in one kernel
      if (i == NL - 1) prof_begin(kProfFrl2, s);   // (the chain of NL - 1 back-to-back launches timed as one)
      const Frl2Layer y{rows, T, mstcn2_dil(p, NL - 1 - i), mstcn2_dil(p, i), q.off, q.nvid, p->dropout,
                        fx_drop_subseed(p->seed, i - 1)};
      FX_TRY(launch_frl2_bwd(y, dCat, ws + L.wk + i * per, ws + L.wk + i * per + c3, gF, dFn,
                             saved + L.r + (i - 1) * L.rowsF, ws + L.du + (i - 1) * L.rowsF,
                             ws + L.wk + (i - 1) * per + 2 * c3, ws + L.dcat + 2 * (i - 1) * L.rowsF, s));
      if (i == 1)
        prof_end(kProfFrl2, s, (NL - 1) * 2.0 * rows * F * 8.0 * F, (NL - 1) * 4.0 * (7.0 * rows * F + 8.0 * F * F),
                 NL - 1);
      gF = dFn;
      continue;
    }
    // dF_i = gF + conv_d1^T(dA) + conv_d2^T(dB)
    for (int h = 0; h < 2; ++h) {
      const int dil = h == 0 ? mstcn2_dil(p, NL - 1 - i) : mstcn2_dil(p, i);
      if (ng > 1) {   // grouped: conv_d1's pass writes gF + conv^T(dA), conv_d2's adds conv^T(dB)
        prof_begin(0, s);
        FX_TRY(launch_gconv(dCat + h * F, 2 * F, rows, T, q.nvid, q.off, F, ng, dil, -1,
                            saved + (h == 0 ? L.wb1 : L.wb2) + i * gsz, nullptr, 0, h == 0 ? gF : nullptr, F, h != 0,
                            dFn, F, s));
        prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (3.0 * rows * F + 3.0 * F * (F / ng)));
        continue;
      }
      fx_gemm_desc d = gemm_desc(rows, F, 3 * F, conv_operand(dCat + h * F, 2 * F, F, dil, -1, q, false),
                                 op_rows(saved + (h == 0 ? L.wb1 : L.wb2) + (long long)i * 3 * F * F, 3 * F), dFn, F);
      if (h == 0) {
        d.resid = gF;
        d.ld_resid = F;
      } else {
        d.beta = 1.f;
      }
      prof_begin(0, s);
      FX_TRY(launch_gemm(d, s));
      prof_end(0, s, 2.0 * rows * F * 3.0 * F, 4.0 * (3.0 * rows * F + 3.0 * F * F));
    }
    gF = dFn;
  }
  // weight gradients of every layer, after the chain (side stream): batched over the layers when the
  // gradient buffers are uniformly strided (views of one flat buffer), else one launch per layer
  FX_TRY(lane.fork(1));
  if (NL > 0) {
    WsBound wbb(ws + L.bsl, L.wk - L.bsl);
    const bool uni = uniform_stride(g->w_fu, NL) && uniform_stride(g->b_fu, NL) && uniform_stride(g->w_d1, NL) &&
                     uniform_stride(g->b_d1, NL) && uniform_stride(g->w_d2, NL) && uniform_stride(g->b_d2, NL);
    const int growth = p->dil_factor > 0 ? p->dil_factor : 2;
    auto st = [&](float* const* v) -> long long { return NL > 1 ? v[1] - v[0] : 0; };
    const int nb = uni ? NL : 1;
    for (int i0 = 0; i0 < NL; i0 += nb) {
      {   // fusion 1x1: dW_fu,i += dU_i^T cat_i, db_fu,i += colsum(dU_i)
        fx_operand a = op_cols(ws + L.du + i0 * L.rowsF, F);
        a.batch_stride = L.rowsF;
        fx_operand b = op_cols(saved + L.cat + 2 * i0 * L.rowsF, 2 * F);
        b.batch_stride = 2 * L.rowsF;
        b.ones_col = 2 * F + 1;
        fx_gemm_desc d = gemm_desc(F, 2 * F + 1, rows, a, b, g->w_fu[i0], 2 * F);
        d.batch = nb;
        d.c_batch_stride = st(g->w_fu);
        d.c_last_col = g->b_fu[i0];
        d.c_last_batch_stride = st(g->b_fu);
        d.beta = 1.f;
        d.split_k = pick_split(F, 2 * F + 1, rows, nb);
        d.workspace = ws + L.bsl;
        FX_TRY(launch_gemm(d, sd));
      }
      for (int h = 0; h < 2 && ng > 1; ++h)   // grouped: one launch per conv and layer of this batch
        for (int il = i0; il < i0 + nb; ++il)
          FX_TRY(launch_gconv_dw(ws + L.dcat + 2 * il * L.rowsF + h * F, 2 * F, saved + L.f + il * L.rowsF, F, rows, T,
                                 q.nvid, q.off, F, ng, mstcn2_dil(p, h == 0 ? NL - 1 - il : il),
                                 (h == 0 ? g->w_d1 : g->w_d2)[il], (h == 0 ? g->b_d1 : g->b_d2)[il], ws + L.bsl, sd));
      for (int h = 0; h < 2 && ng == 1; ++h) {
        // dilated conv h: dW_i += dC_h,i^T taps(f_i), db_i += colsum(dC_h,i); conv_d2's dilation grows with
        // the layer (batch b = layer i0 + b), conv_d1's shrinks: its batch b is layer NL-1-b (negative strides)
        const int il = (h == 0 && uni) ? NL - 1 : i0;
        const long long dir = (h == 0 && uni) ? -1 : 1;
        const int dil = h == 0 ? mstcn2_dil(p, NL - 1 - il) : mstcn2_dil(p, il);
        float* const* gw = h == 0 ? g->w_d1 : g->w_d2;
        float* const* gb = h == 0 ? g->b_d1 : g->b_d2;
        FX_TRY(per_video(q, [&](int r0, int nr, const Seqs& qv) -> int {
          fx_operand a = op_cols(ws + L.dcat + 2 * il * L.rowsF + (long long)r0 * 2 * F + h * F, 2 * F);
          a.batch_stride = dir * 2 * L.rowsF;
          fx_operand b = conv_operand(saved + L.f + il * L.rowsF + (long long)r0 * F, F, F, dil, 1, qv, true);
          b.batch_stride = dir * L.rowsF;
          b.ones_col = 3 * F + 1;
          fx_gemm_desc d = gemm_desc(F, 3 * F + 1, nr, a, b, gw[il], 3 * F);
          d.batch = nb;
          d.c_batch_stride = dir * st(gw);
          d.c_last_col = gb[il];
          d.c_last_batch_stride = dir * st(gb);
          d.b_dil_growth = nb > 1 ? growth : 0;
          d.c_tap_cin = F;
          d.beta = 1.f;
          d.split_k = pick_split(F, 3 * F + 1, nr, nb);
          d.workspace = ws + L.bsl;
          return launch_gemm(d, sd);
        }));
      }
    }
  }
  if (p->in_map) {
    if (g->w_in) {
      FX_TRY(lane.fork(2));
      WsBound wb(spl, L.bsl - L.spl);
      FX_TRY(linear_dwdb(gF, F, x, ldx, rows, p->cin, F, g->w_in, g->b_in, 1, spl, sd));
    }
    if (dx) FX_TRY(linear_dx(gF, F, p->w_in, rows, p->cin, F, dx, lddx, 0, nullptr, 0, spm, s));
  } else if (dx) {
    FX_CHECK_HIP(hipMemcpy2DAsync(dx, lddx * sizeof(float), gF, F * sizeof(float), F * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, s));
  }
  return lane.join(p->side_defer);
}

// ---------------------------------------------------------------- grouped dilated conv, one layer
// workspace: [forward image | dX image | weight-gradient partials]
long long fx_conv3g_workspace_floats(int rows, int F, int ngroup) {
  if (F < 1 || ngroup < 0 || F % std::max(ngroup, 1) != 0) return 0;
  return 2 * al64(gconv_packed_floats(F, ngroup)) + gconv_dw_ws_floats(rows, F, ngroup);
}

int fx_conv3g_fwd(const float* x, long long ldx, int rows, int T, int nvid, const int* seq_off, int F, int ngroup,
                  int dil, const float* w, const float* b, int relu, float* y, long long ldy, float* workspace,
                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_TRY(gconv_check(F, ngroup, "fx_conv3g_fwd"));
  FX_REQUIRE(x && w && y && workspace && rows >= 0 && dil >= 1, "fx_conv3g_fwd: bad arguments");
  const int ng = std::max(ngroup, 1);
  float* wf = workspace;
  float* wb = wf + al64(gconv_packed_floats(F, ng));
  const GPackJob job{w, wf, wb, nullptr, nullptr};
  FX_TRY(launch_gconv_pack(&job, 1, F, ng, s));
  prof_begin(0, s);
  const int st = launch_gconv(x, ldx, rows, T, nvid, seq_off, F, ng, dil, 1, wf, b, relu, nullptr, 0, 0, y, ldy, s);
  prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (2.0 * rows * F + 3.0 * F * (F / ng)));
  return st;
}

int fx_conv3g_bwd(const float* x, long long ldx, int rows, int T, int nvid, const int* seq_off, int F, int ngroup,
                  int dil, const float* w, const float* dy, long long lddy, float* dx, long long lddx, float* dw,
                  float* db, float* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FX_TRY(gconv_check(F, ngroup, "fx_conv3g_bwd"));
  FX_REQUIRE(x && w && dy && workspace && rows >= 0 && dil >= 1, "fx_conv3g_bwd: bad arguments");
  const int ng = std::max(ngroup, 1);
  float* wf = workspace;
  float* wb = wf + al64(gconv_packed_floats(F, ng));
  float* part = wb + al64(gconv_packed_floats(F, ng));
  if (dx) {
    const GPackJob job{w, wf, wb, nullptr, nullptr};
    FX_TRY(launch_gconv_pack(&job, 1, F, ng, s));
    prof_begin(0, s);
    const int st = launch_gconv(dy, lddy, rows, T, nvid, seq_off, F, ng, dil, -1, wb, nullptr, 0, nullptr, 0, 0, dx,
                                lddx, s);
    prof_end(0, s, 2.0 * rows * F * 3.0 * (F / ng), 4.0 * (2.0 * rows * F + 3.0 * F * (F / ng)));
    FX_TRY(st);
  }
  if (dw || db) FX_TRY(launch_gconv_dw(dy, lddy, x, ldx, rows, T, nvid, seq_off, F, ng, dil, dw, db, part, s));
  return FX_OK;
}

}  // extern "C"
