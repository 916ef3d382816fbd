// Frame-level helpers shared by the MS-TCN and MS-TCN++ translation units (mstcn.cpp, mstcn2.cpp).
#pragma once
#include "fx_common.h"
#include "ops.h"

namespace fx {

// groups of the dilated convs: fx_mstcn_params.ngroup / fx_mstcn2_params.ngroup (0 and 1: dense; an invalid
// count sizes as dense -- the entry points refuse it)
inline int mstcn_groups(int ngroup, int F) { return ngroup > 1 && F > 0 && F % ngroup == 0 ? ngroup : 1; }

// The videos of a frame-level call: nvid of T rows each, or ragged host offsets off (nvid + 1).
struct Seqs {
  int T, nvid;
  const int* off;
  int rows() const { return off ? off[nvid] : T * nvid; }
  int start(int v) const { return off ? off[v] : v * T; }
  int len(int v) const { return off ? off[v + 1] - off[v] : T; }
};

inline int check_seqs(const Seqs& q) {
  FX_REQUIRE(q.nvid >= 1, "frame branch: nvid >= 1");
  if (!q.off) {
    FX_REQUIRE(q.T >= 1, "frame branch: T >= 1");
    return FX_OK;
  }
  FX_REQUIRE(q.nvid <= 16 && q.off[0] == 0, "frame branch: ragged offsets start at 0, <= 16 videos");
  for (int v = 0; v < q.nvid; ++v) FX_REQUIRE(q.off[v + 1] > q.off[v], "frame branch: empty video");
  return FX_OK;
}

// dilated-conv operand over the call's videos (zero outside each video).  The column-major (weight-
// gradient) form of a ragged call needs K padded to whole 64-deep stages (gemm_dev.h COLS_CONVR): the
// per-layer weight gradients (K = rows) run video by video instead.
inline fx_operand conv_operand(const float* h, long long ld, int cin, int dil, int dir, const Seqs& q, bool trans) {
  fx_operand o = trans ? op_cols(h, ld) : op_rows(h, ld);
  o.conv_taps = 3;
  o.conv_cin = cin;
  o.conv_dil = dil;
  o.conv_dir = dir;
  if (q.off) {   // (column-major: FAST loaders only, K padded to whole stages -- the deferred dW GEMMs)
    o.seq_off = q.off;
    o.nseq = q.nvid;
  } else {
    o.seq_len = q.T;
  }
  return o;
}

// fn(row0, rows, seqs) once over all rows (uniform videos) or once per video (ragged): the weight-
// gradient GEMMs whose K runs over frames
template <typename Fn>
int per_video(const Seqs& q, Fn fn) {
  if (!q.off) return fn(0, q.rows(), q);
  for (int v = 0; v < q.nvid; ++v) FX_TRY(fn(q.start(v), q.len(v), Seqs{q.len(v), 1, nullptr}));
  return FX_OK;
}

// whether the n per-layer gradient pointers are all set and layer i's is layer 0's plus i times one stride
// (views of one flat gradient buffer in parameter order: FlatGradReducer) -- what a weight-gradient GEMM
// batched over the layers needs
inline bool uniform_stride(float* const* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!v[i]) return false;
  for (int i = 2; i < n; ++i)
    if (v[i] - v[i - 1] != v[1] - v[0]) return false;
  return true;
}

// NL conv weights (F, F / ng, 3) -> forward images at wf and input-gradient images at wb (one packed image
// per layer: pack_conv_kernel, or conv_grouped.hip's when ng > 1); optionally the 1x1 weights wpw[l] (F, F)
// transposed into wpt + l F F (mstcn.cpp)
int pack_conv_set(const float* const* w, int NL, int F, int ng, float* wf, float* wb, const float* const* wpw,
                  float* wpt, hipStream_t s);

}  // namespace fx
