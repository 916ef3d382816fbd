// The GEMM planner: from a descriptor, the caller's precision and the knobs to a GemmPlan.  It only
// plans -- no stream, no allocation, no runtime call -- so every decision can be read (and tested) here.
#include <algorithm>

#include "gemm_plan.h"

namespace fx {
namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Small problems go to the direct kernel: token-level (M or N <= 64: the Nact tokens of one or two
// lockstep videos) or shallow K.  (Few-tile frame-level dW GEMMs with K = T stay tiled: measured
// 25 vs 32 us at 256x257x4096.)  Conv-gather operands always take the tiled kernel.
// FX_GEMM_PATH=tiled|direct overrides the choice (diagnostic).
bool use_direct(const fx_gemm_desc& d, int ak, int bk, const Knobs& kn) {
  const int force = kn.gemm_path;
  // the direct kernel addresses ROWS / COLS operands with 32-bit byte offsets (dload)
  auto fits = [&](const fx_operand& o, int kind, int R) {
    const double k = (double)d.K + 2 * DMAXW * DCH + 64, ld = (double)o.ld;
    const double bytes = kind == ROWS ? ((double)R * ld + k) * 4 : kind == COLS ? (k * ld + R) * 4 : 0;
    return bytes < 4294967296.0;
  };
  const bool ok = d.K > 0 && direct_pair(gen_kind(ak), bk) && fits(d.a, ak, d.M) && fits(d.b, bk, d.N);
  if (!ok || force == 1) return false;
  if (force == 2) return true;
  // gathered A rows (ROWS_GEN / ROWS_CAT) load element by element in the direct kernel: only the
  // 32-row case pays off there (64 x 256 x 1024 concat: 54 us direct vs 29 us tiled)
  const int lim = (ak == ROWS_GEN || ak == ROWS_CAT) ? 32 : 64;
  // a shallow K that is not a whole number of 64-deep stages would take the generic tiled kernel
  // (InfoNCE dF: 4096 x 512 x 70, 80 us there; Breakfast's token dW over 4 x 60 = 240 token rows,
  // 512 x 513 x 240: 61 us there); one pass of the direct kernel per tile is ~10x faster
  if (d.M <= lim || d.N <= lim || d.K <= 64 || (d.K <= 512 && d.K % 64 != 0)) return true;
  // few output tiles (the TDU blocks' segment-level products: S ~ 50-250 segment rows per launch): the
  // tiled kernel's fixed cost -- a 64-deep stage pipeline filled per block, one 64 x 64 block per ~4 tiles
  // of 32 x 32 -- is most of its time there; the direct kernel runs every 32 x 32 tile's K chunks on
  // their own waves.  Measured (tools/r06_seg_gemm.py, SWEEP=1): 192 x 512 x 512 7.9 vs 16.0 us (tiled,
  // 12.8 with split 4), 1024 x 256 x 512 7.9 vs 16.1, 1024 x 512 x 512 14.0 vs 16.4, 192 x 512 x 2048
  // 19.5 vs 20.2 (split 4); past ~512 tiles the tiled kernel wins (1536 x 512 x 512: 20.1 vs 16.7)
  const long long t32 = (long long)cdiv(d.M, 32) * cdiv(d.N, 32) * d.batch;
  return (ak == ROWS || ak == COLS) && t32 <= 512 && d.K <= 2048;
}

// 128x64 tiles where the launch still has ~3/4 of a block per CU: FAST operands only.
// FX_GEMM_WIDE=0|1 forces the choice among eligible launches (diagnostic).
bool use_wide(const GemmDev& g, int ak, int bk, int batch, const Knobs& kn) {
  const int force = kn.gemm_wide;
  const bool fast = g.a_vec && g.b_vec && ((g.K % BK) == 0 || ak == COLS_KT);
  const bool ok = fast && wide8_pair(ak, bk);
  if (!ok || force == 0) return false;
  if (force == 1) return true;
  return (long long)cdiv(g.M, WBM) * g.tiles_x * batch * g.split >= 192;
}

}  // namespace

bool operand_vec_ok(const fx_operand& o) {
  if (!aligned16(o.ptr) || (o.ld & 3)) return false;
  if (o.batch_stride & 3) return false;
  if (o.conv_taps && (o.conv_cin & 7)) return false;
  if (!o.trans && o.ptr1 && (!aligned16(o.ptr1) || (o.ld1 & 3) || (o.k_split & 7))) return false;
  return true;
}

int kind_of(const fx_operand& o, bool vec) {
  if (o.trans) return o.conv_taps ? (o.nseq > 0 ? COLS_CONVR : COLS_CONV) : COLS;
  if (o.conv_taps) return (vec && o.conv_cin % BK == 0) ? ROWS_CONV : ROWS_GEN;   // a stage stays in one tap
  if (o.pos) return ROWS_GEN;
  if (o.ptr1 || o.rows0 || o.rows1) return (vec && (!o.ptr1 || o.k_split % BK == 0)) ? ROWS_CAT : ROWS_GEN;
  return ROWS;
}

int plan_gemm(const fx_gemm_desc& d, int prec, const Knobs& kn, long long tile_cnt_base, GemmPlan& P) {
  FX_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0 && d.batch >= 1, "gemm: bad sizes");
  FX_REQUIRE(d.a.ptr && d.b.ptr && d.c, "gemm: null operand");
  FX_REQUIRE(!(d.a.conv_taps && d.a.seq_len <= 0 && d.a.nseq <= 0) &&
                 !(d.b.conv_taps && d.b.seq_len <= 0 && d.b.nseq <= 0),
             "gemm: conv operand needs seq_len or seq_off");
  FX_REQUIRE(d.a.nseq <= 0 || !d.a.trans, "gemm: ragged conv offsets on a row-major A or a column-major B operand");
  FX_REQUIRE(d.b.nseq <= 0 || (d.b.trans && d.b.conv_taps && d.a.nseq <= 0),
             "gemm: ragged column-major conv B needs a plain A operand");
  FX_REQUIRE(!(d.a.conv_taps && d.K != d.a.conv_taps * d.a.conv_cin), "gemm: conv A needs K == taps*cin");
  FX_REQUIRE(!(d.b.conv_taps && d.b.trans && d.N != d.b.conv_taps * d.b.conv_cin + (d.b.ones_col ? 1 : 0)),
             "gemm: conv B needs N == taps*cin (+1 with a ones column)");
  FX_REQUIRE(!(d.a.ones_col && !d.a.trans) && !(d.b.ones_col && !d.b.trans), "gemm: ones_col needs trans==1");
  FX_REQUIRE(!(d.b.conv_taps && !d.b.trans), "gemm: row-major conv B operand is not supported");
  P = GemmPlan{};
  GemmDev& g = P.g;
  g.M = d.M;
  g.N = d.N;
  g.K = d.K;
  g.a = d.a;
  g.b = d.b;
  {   // ragged conv videos: the offsets travel in the kernel arguments
    const fx_operand& o = d.a;
    if (o.nseq > 0) {
      FX_REQUIRE(o.conv_taps && o.seq_off && o.nseq <= kMaxSeq, "gemm: seq_off needs a conv operand, <= 16 videos");
      const int rows = d.M;
      FX_REQUIRE(o.seq_off[0] == 0 && o.seq_off[o.nseq] == rows, "gemm: seq_off must span the operand's rows");
      for (int v = 0; v <= o.nseq; ++v) {
        FX_REQUIRE(v == 0 || o.seq_off[v] > o.seq_off[v - 1], "gemm: seq_off must increase");
        g.soff[v] = o.seq_off[v];
      }
      g.nsoff = o.nseq;
    }
  }
  {   // ragged column-major conv B (weight gradients of a ragged batch, K = frames): K may pad the last
      // video to whole 64-deep stages; those frames read as zero
    const fx_operand& o = d.b;
    if (o.nseq > 0) {
      FX_REQUIRE(o.seq_off && o.nseq <= kMaxSeq && o.seq_off[0] == 0 && o.seq_off[o.nseq] <= d.K,
                 "gemm: ragged B offsets must start at 0 and end within K, <= 16 videos");
      FX_REQUIRE(operand_vec_ok(d.a) && operand_vec_ok(d.b) && d.K % BK == 0,
                 "gemm: ragged B needs 16-B operands and K a multiple of 64 (pad the frames)");
      for (int v = 0; v <= kMaxSeq; ++v) {
        FX_REQUIRE(v == 0 || v > o.nseq || o.seq_off[v] > o.seq_off[v - 1], "gemm: seq_off must increase");
        g.soff[v] = v <= o.nseq ? o.seq_off[v] : 0x7fffffff;
      }
      g.nsoff = o.nseq;
    }
  }
  g.c = d.c;
  g.ldc = d.ldc;
  g.c_bs = d.c_batch_stride;
  g.alpha = d.alpha;
  g.beta = d.beta;
  g.bias = d.bias;
  g.resid = d.resid;
  g.ld_resid = d.ld_resid;
  g.resid_bs = d.resid_batch_stride;
  g.gate = d.gate;
  g.ld_gate = d.ld_gate;
  g.relu = d.relu;
  g.c_tap_cin = d.c_tap_cin;
  g.c_last = d.c_last_col;
  g.c_last_bs = d.c_last_batch_stride ? d.c_last_batch_stride : d.M;
  g.b_dil_growth = d.b_dil_growth;
  g.a_dil_b1 = d.a_dil_b1;
  g.bias_bs = d.bias_batch_stride;
  FX_REQUIRE(d.a_dil_b1 <= 0 || (d.a.conv_taps && !d.a.trans), "gemm: a_dil_b1 needs a row-major conv A");
  FX_REQUIRE(d.b_dil_growth <= 1 || (d.b.conv_taps && d.b.trans), "gemm: b_dil_growth needs a column-major conv B");
  g.stamps = d.dbg_stamps;
  FX_REQUIRE(d.drop_p >= 0.f && d.drop_p < 1.f, "gemm: dropout p must be in [0, 1)");
  FX_REQUIRE(d.drop_p == 0.f || (!d.c_last_col && !d.c_tap_cin && !d.gate && d.beta == 0.f &&
                                 !(d.relu == 1 && d.resid)),
             "gemm: dropout only on plain outputs (before the residual add)");
  g.drop_thr = d.drop_p > 0.f ? std::max(fx_drop_thresh(d.drop_p), 1u) : 0u;
  g.drop_scale = 1.f / (1.f - d.drop_p);
  g.drop_seed = d.drop_seed;
  g.a_vec = operand_vec_ok(d.a);
  g.b_vec = operand_vec_ok(d.b);
  g.ws = d.workspace;
  int ak = kind_of(d.a, g.a_vec), bk = kind_of(d.b, g.b_vec);
  const bool direct = d.b_dil_growth <= 1 && d.a_dil_b1 <= 0 && use_direct(d, ak, bk, kn);   // (the direct kernel: one dilation)
  // weight gradients over a frame count that is not a whole number of 64-deep stages (ragged batches):
  // the K-tail loaders keep them on the FAST tiled / wide kernels instead of the element-wise generic one
  if (!direct && ak == COLS && bk == COLS && g.a_vec && g.b_vec && d.K % BK != 0 && kn.gemm_ktail) ak = bk = COLS_KT;
  P.ak = ak;
  P.bk = bk;
  P.batch = d.batch;
  bool wide = false;
  const int cap = (d.split_k > 1 && d.workspace) ? d.split_k : 1;   // workspace holds `cap` slabs
  FX_REQUIRE(!(d.split_k > 1 && !d.workspace), "gemm: split-K needs a workspace");
  if (direct) {
    const int nch = cdiv(d.K, DCH);
    const long long t32 = (long long)cdiv(d.M, 32) * cdiv(d.N, 32) * d.batch;
    // one 32-deep k chunk per wave, up to 8 waves per tile (two chunks per wave measured slower: round 3)
    const int cpw = 1;
    const int nw = std::min(DMAXW, std::max(1, nch / cpw));
    int split = 1;
    // split K only for launches of few tiles (the token rows): from 64 tiles up the extra slabs and the
    // last arriver's reduction cost more than they spread (102 x 512 x 512: 7.8 us unsplit, 9.7 in 4)
    if (cap > 1 && t32 < 64) {
      const long long want = std::min<long long>(nch / (cpw * nw), cdiv(2048, t32 * nw));
      split = (int)std::max<long long>(1, std::min<long long>(cap, want));
    }
    g.kt_per_split = nch > 0 ? cdiv(nch, split) : 0;
    g.split = g.kt_per_split > 0 ? cdiv(nch, g.kt_per_split) : 1;
    g.tiles_x = cdiv(d.N, 32);
    g.tiles_y = cdiv(d.M, 32);
    P.block = dim3(nw * 64);
  } else {
    const int nkt = cdiv(d.K, BK);
    int split = std::min(cap, std::max(nkt, 1));
    g.kt_per_split = nkt > 0 ? cdiv(nkt, split) : 0;
    g.split = g.kt_per_split > 0 ? cdiv(nkt, g.kt_per_split) : 1;
    g.tiles_x = cdiv(d.N, BN);
    wide = use_wide(g, ak, bk, d.batch, kn);
    g.tiles_y = cdiv(d.M, wide ? WBM : BM);
    P.block = dim3(wide ? W8T : NTHREADS);
  }
  P.grid = dim3(g.tiles_x, g.tiles_y, d.batch * g.split);
  // the family: the precision modes take the 128x64-tile launches with row-major A; everything else
  // (weight gradients: A column-major; direct / small tiles) keeps the f32 MFMA kernels
  const bool lowp = wide && bf16_pair(ak, bk);
  P.np = !lowp ? 0 : prec == FX_PREC_F32S ? 3 : prec == FX_PREC_F32S2 ? 2 : 0;
  P.family = direct ? FAM_DIRECT
           : !wide ? FAM_TILED
           : P.np ? (split_pair(ak, bk) ? FAM_SPLIT : FAM_WIDE8)
           : (lowp && prec == FX_PREC_BF16) ? FAM_BF16
                                            : FAM_WIDE8;
  // FAST loop: both operands 16-B vector-loadable, K a multiple of the 64-deep stage, no gathers
  P.fast = P.family == FAM_TILED && g.a_vec && g.b_vec && ((g.K % BK) == 0 || ak == COLS_KT) && ak != ROWS_GEN &&
           gen_kind(bk) != ROWS_GEN;
  const bool runs = P.family == FAM_DIRECT  ? direct_pair(gen_kind(ak), bk)
                    : P.family == FAM_TILED ? tiled_pair(ak, gen_kind(bk), P.fast)
                    : P.family == FAM_BF16  ? bf16_pair(ak, bk)
                    : P.family == FAM_SPLIT ? split_pair(ak, bk)
                    : P.np                  ? wide8_split_pair(ak, bk)
                                            : wide8_pair(ak, bk);
  if (!runs) {
    set_error("gemm: unsupported operand kinds");
    return FX_ERR_UNSUPPORTED;
  }
  // in-launch reduction only while the last block's serial slab read stays small (<= 32 KB per
  // tile); bigger ones pay less as a separate reduce launch (conv dW split 5: 78 vs 56 us)
  const long long slab_bytes = (long long)g.split * (direct ? 32 * 32 : (wide ? WBM : BM) * BN) * 4;
  const long long tiles = (long long)g.tiles_x * g.tiles_y * d.batch;
  P.cnt_base = tile_cnt_base;
  P.counters = (g.split > 1 && slab_bytes <= 32768 && tile_cnt_base + tiles <= kArrivalCounters) ? tiles : 0;
  // FX_GEMM_XCDPLANES=0: the per-plane tile mapping for every launch (A/B)
  const long long nz = (long long)d.batch * g.split;
  g.xcd_planes = kn.gemm_xcd_planes && wide && nz >= 8 && nz % 8 == 0;
  // FX_GEMM_ROWPERM=0: keep row tiles in order for dilated-conv A operands too (A/B)
  if (kn.gemm_row_perm && wide && !g.xcd_planes && d.a.conv_taps > 1 && !d.a.trans && d.a_dil_b1 <= 0) {
    const int sh = d.a.conv_dil / WBM;
    if (sh > 1 && g.tiles_y % sh == 0) g.row_perm = sh;
  }
  // FX_GEMM_GROUPM=0: plain row-major tile runs (A/B).  Grouped order when B does not fit an XCD's L2
  // share (> 2 MB) but one XCD run of A rows does (<= 2 MB), plain operands only
  if (kn.gemm_group_m && !g.xcd_planes && g.row_perm <= 1 && d.a.conv_taps <= 1 && d.b.conv_taps <= 1 &&
      g.tiles_y >= 16 && g.tiles_x >= 8) {
    const int gm = g.tiles_y / 8, tm = wide ? WBM : BM;
    const double b_bytes = 4.0 * d.N * d.K, a_run = 4.0 * gm * tm * d.K;
    if (b_bytes > 2.0 * (1 << 20) && a_run <= 2.0 * (1 << 20)) g.group_m = gm;
  }
  // FX_GEMM_PERSIST=0: one workgroup per tile (A/B).  A persistent grid for the f32 wide8 kernel on
  // single, unsplit products with at least two tiles per CU (the kernel loops over virtual workgroups)
  if (kn.gemm_persist && P.family == FAM_WIDE8 && !P.np && g.split == 1 && d.batch == 1 && !g.xcd_planes) {
    const long long nt = (long long)g.tiles_x * g.tiles_y;
    constexpr int G = 256;   // (a multiple of 8: a virtual workgroup keeps its physical one's XCD)
    if (nt >= 2 * G) {
      g.persist = (int)nt;
      P.grid = dim3(G, 1, 1);
    }
  }
  return FX_OK;
}

}  // namespace fx
