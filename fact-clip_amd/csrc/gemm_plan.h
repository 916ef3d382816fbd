// What a GEMM launch is before it is launched: the plan (operand kinds, kernel family, tiles, split,
// grid), the statement of which operand kinds each kernel family runs, and the one dispatcher that
// turns run-time kinds into a kernel instantiation.
//
// A family's pairs are stated ONCE, as a constexpr predicate.  The planner calls it at run time (a
// pair outside it is FX_ERR_UNSUPPORTED before anything is launched); the family's launcher hands it
// to dispatch_pair, which instantiates the kernel for exactly the pairs it accepts.  A new family is
// one .hip file, one predicate, one Family value and one row in launch_family (gemm.cpp).
#pragma once
#include <type_traits>
#include <utility>

#include "gemm_dev.h"

namespace fx {

enum Family { FAM_TILED = 0, FAM_WIDE8, FAM_BF16, FAM_SPLIT, FAM_DIRECT };

// ---------------------------------------------------------------- which pairs a family runs
// ROWS_CAT has a FAST loader as the A operand of the LDS-tiled kernels only; as a tiled B and as a
// direct A the concatenation runs on the generic element fetch
constexpr int gen_kind(int k) { return k == ROWS_CAT ? ROWS_GEN : k; }

constexpr bool rowmajor_a(int ak) { return ak == ROWS || ak == ROWS_CONV || ak == ROWS_CAT; }

// 64x64 tiles (gemm_tiled.hip); bk after gen_kind.  FAST: see Loader.  The ragged conv B and the
// K-tail pair exist as FAST loaders only; the generic fetch takes every row-major form
constexpr bool tiled_pair(int ak, int bk, bool fast) {
  const bool a = rowmajor_a(ak) || ak == COLS || ak == COLS_KT || (ak == ROWS_GEN && !fast);
  const bool b = bk == ROWS || bk == COLS || bk == COLS_CONV || (bk == ROWS_GEN && !fast) ||
                 (fast && ((bk == COLS_CONVR && ak == COLS) || (bk == COLS_KT && ak == COLS_KT)));
  return a && b;
}
constexpr bool tiled_fast_pair(int ak, int bk) { return tiled_pair(ak, bk, true); }
constexpr bool tiled_generic_pair(int ak, int bk) { return tiled_pair(ak, bk, false); }

// 128x64 tiles, 8 waves, f32 MFMA (gemm_wide8.hip): FAST operands only
constexpr bool wide8_pair(int ak, int bk) { return tiled_pair(ak, bk, true); }

// FX_PREC_BF16 / FX_PREC_F32S / FX_PREC_F32S2 on the 128x64 tile: row-major A (forward and input-gradient
// products); weight gradients (A column-major) keep the f32 MFMA
constexpr bool bf16_pair(int ak, int bk) { return rowmajor_a(ak) && (bk == ROWS || bk == COLS); }
// fp32 by split bf16: B row-major splits in registers (the wide8 kernel's NP = 2 / 3 forms), B column-major
// through split LDS images (gemm_split.hip)
constexpr bool wide8_split_pair(int ak, int bk) { return rowmajor_a(ak) && bk == ROWS; }
constexpr bool split_pair(int ak, int bk) { return rowmajor_a(ak) && bk == COLS; }

// small shapes (gemm_direct.hip); ak after gen_kind
constexpr bool direct_pair(int ak, int bk) {
  return (ak == ROWS || ak == ROWS_GEN || ak == COLS) && (bk == ROWS || bk == COLS);
}

// ---------------------------------------------------------------- the plan
struct GemmPlan {
  GemmDev g;           // the kernel argument (tile_cnt is attached by the launcher, see counters)
  dim3 grid, block;
  int ak, bk;          // operand kinds (kind_of)
  int family;
  bool fast;           // FAM_TILED: the FAST loaders
  int np;              // FAM_WIDE8 / FAM_SPLIT: bf16 pieces per fp32 operand (0: f32 MFMA)
  int batch;
  // in-launch split-K reduction wanted: arrival counters [cnt_base, cnt_base + counters) of the stream's
  // pool, one per output tile (0: a separate reduce launch follows a split launch)
  long long cnt_base, counters;
};

bool operand_vec_ok(const fx_operand& o);
int kind_of(const fx_operand& o, bool vec);

// Everything decided before a GEMM is launched.  prec: the caller stream's FX_PREC_*; tile_cnt_base: the
// first arrival counter this launch may use (the members of one grouped launch get disjoint ranges).
// Pure: no stream, no allocation, nothing from the HIP runtime.
int plan_gemm(const fx_gemm_desc& d, int prec, const Knobs& k, long long tile_cnt_base, GemmPlan& P);

// ---------------------------------------------------------------- the launchers (one per family file)
int launch_tiled(const GemmPlan& P, hipStream_t s);
int launch_wide8(const GemmPlan& P, hipStream_t s);
int launch_bf16(const GemmPlan& P, hipStream_t s);
int launch_split(const GemmPlan& P, hipStream_t s);
int launch_direct(const GemmPlan& P, hipStream_t s);
void launch_direct_group(const GemmGroup& G, int blocks, unsigned threads, hipStream_t s);
// the separate split-K reduce of a split launch that got no arrival counters
int launch_reduce(const GemmPlan& P, hipStream_t s);

// ---------------------------------------------------------------- kind dispatch
// f(std::integral_constant<int, K>) for the Kind K equal to k
template <class F, int... Ks>
void with_kind(int k, F&& f, std::integer_sequence<int, Ks...>) {
  ((k == Ks ? f(std::integral_constant<int, Ks>{}) : void()), ...);
}
using AllKinds = std::integer_sequence<int, ROWS, ROWS_CONV, ROWS_GEN, COLS, COLS_CONV, ROWS_CAT, COLS_CONVR, COLS_KT>;

// launch(A, B) with the kinds as integral constants, instantiated for the pairs Pair accepts and no others
template <bool (*Pair)(int, int), class F>
int dispatch_pair(int ak, int bk, const char* family, F&& launch) {
  bool done = false;
  with_kind(ak, [&](auto A) {
    with_kind(bk, [&](auto B) {
      if constexpr (Pair(decltype(A)::value, decltype(B)::value)) {
        launch(A, B);
        done = true;
      }
    }, AllKinds{});
  }, AllKinds{});
  if (done) return FX_OK;
  set_error(std::string("gemm(") + family + "): unsupported operand kinds");
  return FX_ERR_UNSUPPORTED;
}

}  // namespace fx
