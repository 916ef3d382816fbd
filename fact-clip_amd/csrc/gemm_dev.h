// f32 GEMM on CDNA4 matrix cores: v_mfma_f32_32x32x2_f32 (exact f32 products,
// k-ordered fma chain; no xf32 on gfx950, so the parity path stays fp32).
//
// One kernel template covers every dense contraction of the FACT frame/action
// branches; the operand loader is specialised at compile time:
//   ROWS      element (r,k) = p[r*ld + k]            Linear/Conv1d(k=1) fwd, B = W
//   ROWS_CONV implicit dilated Conv1d(k=3): row r shifted by the tap of k, zero
//             outside the video (fwd and, with reversed taps, dX)
//   ROWS_GEN  concatenated inputs / row gathers / positional adds (generic)
//   COLS      element (r,k) = p[k*ld + r]            dY^T for dW, W^T for dX
//   COLS_CONV conv input for dW, tap from r; optional all-ones row (bias grad)
//   COLS_CONVR the same over ragged videos (host row offsets): weight gradients of a ragged batch in
//             one launch, K padded to whole stages (rows past the last video read as zero)
//   COLS_KT   COLS with K not a whole number of 64-deep stages (frame-level weight gradients over a
//             ragged frame count): rows past K read as zero from a clamped address, both operands
//
// Tiled kernel: 64x64 output tile per 256-thread workgroup, one wave per SIMD, each wave a
// 32x32 sub-tile over the block's whole K range (32 MFMAs = 2048 matrix-core cycles per
// 64-deep stage between barriers).  K is staged through a 3-slot LDS ring: stage s+2 is
// written while stage s is multiplied, so the fragments of stage s+1 are already visible
// when a wave reaches the end of stage s and one barrier per stage suffices.  Global loads
// run one more stage ahead in two register sets.  Inside a stage each lane works on 32
// CONSECUTIVE k (lane half h takes k in [32h, 32h+32)): A and B agree on that order, which is
// all an MFMA chain needs, and it lets row-major images be read as ds_read_b128 (4 MFMAs of
// operand per read) and written as ds_write_b128 straight from the float4 global loads.
//   row-major kinds -> LDS image [row][k], stride 68 (16-B rows; b128 reads conflict-free)
//   col-major kinds -> LDS image [k][row], stride 65 (b32 reads conflict-free over 64 lanes)
// Blocks are remapped so that consecutive output tiles share an XCD (L2).
//
// This header is the device side that more than one kernel family uses: the kernel argument, the
// operand loaders, the epilogue and the tile order.  One family per file: gemm_tiled.hip (64x64),
// gemm_wide8.hip (128x64, 8 waves), gemm_bf16.hip, gemm_split.hip, gemm_direct.hip (small shapes),
// gemm_reduce.hip (split-K reduce, column sums); gemm_plan.h says which family runs which operands.
#pragma once
#include "fx_common.h"
#include "wave_dev.h"

namespace fx {

constexpr int BM = 64, BN = 64, BK = 64, NTHREADS = 256;
constexpr int RS = 68;              // [row][k] image stride
constexpr int CS = 65;              // [k][row] image stride
constexpr int IMG = BM * RS;        // floats per operand image (>= BK * CS)
constexpr int NSLOT = 3;            // LDS ring depth
constexpr int WBM = 128;            // rows of the wide (128 x 64) tile
constexpr int W8T = 512;            // threads of the 8-wave kernels on it
constexpr int DCH = 32, DMAXW = 8;  // direct kernel: k per chunk, waves per 32x32 tile at most
#define FX_INLINE __attribute__((always_inline))

// ROWS_CAT: [src0[rows0[r]] | src1[rows1[r]]] split at k_split (a multiple of the 64-deep stage),
//           either gather optional -- the FAST form of the concatenation / gather operands
constexpr int kMaxSeq = 16;        // ragged videos per conv operand

enum Kind { ROWS = 0, ROWS_CONV = 1, ROWS_GEN = 2, COLS = 3, COLS_CONV = 4, ROWS_CAT = 5, COLS_CONVR = 6, COLS_KT = 7 };

struct GemmDev {
  int M, N, K;
  fx_operand a, b;
  float* c;
  long long ldc, c_bs;
  float alpha, beta;
  const float* bias;
  const float* resid;
  long long ld_resid, resid_bs;
  const float* gate;
  long long ld_gate;
  int relu, split, kt_per_split, a_vec, b_vec, c_tap_cin;
  float* ws;
  float* c_last;
  int tiles_x, tiles_y;
  long long* stamps;
  unsigned* tile_cnt;   // split-K arrival counters (one per output tile), NULL -> separate reduce kernel
  unsigned drop_thr;    // dropout (fx_drop_bits >= drop_thr keeps); 0 = off
  float drop_scale;
  unsigned long long drop_seed;
  long long c_last_bs;  // c_last of batch b at c_last + b * c_last_bs
  int b_dil_growth;     // > 1: B's conv dilation of batch b is conv_dil * growth^b
  int xcd_planes;       // wide8: whole z-planes (batch x split-K slice) per XCD, see block_tile
  int row_perm;         // > 1: dilated-conv A shifting by row_perm row tiles: XCD runs follow the taps, see block_tile
  int group_m;          // > 1: tiles in groups of group_m row tiles, column-major inside a group, see block_tile
  int persist;          // wide8 only, > 0: tiles per launch; a grid of gridDim.x workgroups walks them (see
                        // gemm_f32_wide8_kernel)
  int a_dil_b1;         // > 0: A's conv dilation of batch 1 (two dilated convs of one input in one launch)
  long long bias_bs;    // bias of batch b at bias + b * bias_bs
  int nsoff;            // > 0: the conv operand's videos are ragged: video v owns rows [soff[v], soff[v+1])
  int soff[kMaxSeq + 1];   // (COLS_CONVR: entries past nsoff are INT_MAX)
};

namespace {

// Position of row r inside its video and the video's length (the conv operand's zero padding):
// uniform videos of seq_len rows, or the ragged offsets soff (nsoff videos; read from the kernel
// arguments, a branch-free count of the video starts at or before r).
typedef int SeqOff[kMaxSeq + 1];

__device__ __forceinline__ void seq_pos(int seq_len, const SeqOff& soff, int nsoff, int r, int& pos, int& len) {
  if (nsoff > 0) {
    // fully unrolled (constant indices: scalar loads from the kernel arguments, no private copy):
    // start = the last offset <= r, end = the first offset > r (offsets increase)
    int start = 0, end = 0x7fffffff;
#pragma unroll
    for (int i = 1; i <= kMaxSeq; ++i) {
      if (i <= nsoff) {
        const int o = soff[i];
        if (o <= r) start = o;
        else end = min(end, o);
      }
    }
    pos = r - start;
    len = end - start;
  } else {
    pos = r % seq_len;
    len = seq_len;
  }
}

// Diagnostic builds (-DFX_STAMPS) record s_memtime / s_memrealtime at fixed points of
// every block; the shipped library compiles the macro to nothing.
#ifdef FX_STAMPS
#define FX_STAMP(g, slot)                                                                          \
  do {                                                                                            \
    if ((g).stamps && threadIdx.x == 0) {                                                         \
      const long long _b = (long long)blockIdx.z * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + \
                           blockIdx.x;                                                            \
      (g).stamps[(_b * 2) * 10 + 2 * (slot)] = __builtin_amdgcn_s_memtime();                       \
      (g).stamps[(_b * 2) * 10 + 2 * (slot) + 1] = __builtin_amdgcn_s_memrealtime();               \
    }                                                                                             \
  } while (0)
#else
#define FX_STAMP(g, slot) \
  do {                    \
  } while (0)
#endif

__device__ __forceinline__ int conv_shift(const fx_operand& o, int tap) {
  return (tap - (o.conv_taps - 1) / 2) * o.conv_dil * o.conv_dir;
}

// A operand of batch bidx: batch 1 may take its own conv dilation (MS-TCN++'s two dilated convs)
__device__ __forceinline__ fx_operand batch_op_a(const fx_operand& a, int dil_b1, int bidx) {
  fx_operand o = a;
  if (dil_b1 > 0 && bidx == 1) o.conv_dil = dil_b1;
  return o;
}

// B operand of batch bidx: a per-batch conv dilation (dilation stacks: layer b's conv_dil * growth^b)
__device__ __forceinline__ fx_operand batch_op_b(const fx_operand& b, int growth, int bidx) {
  fx_operand o = b;
  if (growth > 1)
    for (int i = 0; i < bidx; ++i) o.conv_dil *= growth;
  return o;
}

// ---------------------------------------------------------------- generic element fetch
__device__ __forceinline__ float fetch_rm(const fx_operand& o, const float* p0, int r, int k, const SeqOff& soff,
                                         int nsoff) {
  if (o.conv_taps) {
    const int j = k / o.conv_cin, c = k - j * o.conv_cin, s = conv_shift(o, j);
    int pos, len;
    seq_pos(o.seq_len, soff, nsoff, r, pos, len);
    const int t = pos + s;
    if (t < 0 || t >= len) return 0.f;
    return p0[(long long)(r + s) * o.ld + c];
  }
  if (o.ptr1 && k >= o.k_split) {
    const int rr = o.rows1 ? o.rows1[r] : r;
    return o.ptr1[(long long)rr * o.ld1 + (k - o.k_split)];
  }
  const int rr = o.rows0 ? o.rows0[r] : r;
  float v = p0[(long long)rr * o.ld + k];
  if (o.pos && k < o.pos_cols) v += o.pos[(long long)r * o.ld_pos + k];
  return v;
}

// COLS_CONVR: does frame k + s lie in frame k's video?  Branch-free over the 16 offsets (entries past
// the last video are INT_MAX, so frames past the last video -- the K padding -- are never valid).
__device__ __forceinline__ bool seq_same(const SeqOff& soff, int k, int s) {
  int start = 0, end = 0x7fffffff;
#pragma unroll
  for (int i = 1; i <= kMaxSeq; ++i) {
    const int o = soff[i];
    start = o <= k ? o : start;
    end = o > k ? min(end, o) : end;
  }
  const int t = k + s;
  return end != 0x7fffffff && t >= start && t < end;
}

__device__ __forceinline__ float fetch_cm(const fx_operand& o, const float* p0, int r, int k) {
  if (o.ones_col && r == o.ones_col - 1) return 1.f;
  if (o.conv_taps) {   // uniform videos only (ragged weight gradients run per video)
    const int j = r / o.conv_cin, c = r - j * o.conv_cin, s = conv_shift(o, j);
    const int t = k % o.seq_len + s;
    if (t < 0 || t >= o.seq_len) return 0.f;
    return p0[(long long)(k + s) * o.ld + c];
  }
  return p0[(long long)k * o.ld + r];
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---------------------------------------------------------------- loaders
// A stage is the 64 x 64 (rows x k) tile of one operand; each of the 1024 / NJ threads moves NJ
// float4 of it per stage (NJ = 4: 256-thread blocks, NJ = 2: 512-thread blocks):
//   row-major kinds: rows (tid>>4) + (64/NJ) j, k = (tid&15)*4 .. +3      (j < NJ)
//   col-major kinds: k    (tid>>4) + (64/NJ) j, rows (tid&15)*4 .. +3
// so 16 consecutive threads read one 256-B line.
// FAST (chosen per launch on the host: 16-B aligned operands, K % 64 == 0, no gathers): the
// loads are unconditional straight-line code -- rows past the edge are read from a clamped
// in-range address and replaced by a select (0, or 1 for the virtual ones row) -- so the
// pipelined loop has no bounds branches for the compiler to drain vmcnt at.  !FAST fetches
// element by element with full bounds checks (edge shapes, gathers, concatenations).
// KW = 32 (the split-precision kernel's 32-deep stages, 512 threads, NJ = 1): row-major kinds
// take row tid>>3 and k (tid&7)*4; col-major kinds keep k tid>>4 and rows (tid&15)*4.
template <int KIND, bool FAST, int NJ = 4, int KW = 64>
struct Loader {
  static constexpr int RSTEP = 64 / NJ;   // row (or k) step between a thread's NJ vectors
  static constexpr bool kRowImg = KIND <= ROWS_GEN || KIND == ROWS_CAT;
  fx_operand o;        // by value: the address of a kernel argument would force it to scratch
  const float* base;   // operand base incl. batch offset
  int R, K, r0;
  int ta, tb;          // tid>>4, (tid&15)*4
  int rowc[4];         // row-major: clamped row of j (ROWS_CAT: gathered row of the first source)
  int rowc1[4];        // ROWS_CAT: gathered row of the second source
  int rmod[4];         // ROWS_CONV: position of row j in its video
  int rlen[4];         // ROWS_CONV: that video's length
  SeqOff soff;         // ragged conv videos: a register copy of GemmDev::soff (constant indices only; a
  int nsoff;           // pointer into the kernel arguments would force them into private memory)
  unsigned rok;        // row-major: bit j = row j in range
  int rc;              // col-major: clamped first row of the 4
  unsigned emask, omask;   // col-major: bit e = row rc+e in storage / is the ones row
  int tapc, tap_s;     // COLS_CONV: channel / shift of this thread's 4 rows (one tap: cin % 4 == 0)
  // FAST: per-thread addresses made once, so a stage's load is a uniform offset plus one add per
  // row (the per-row 64-bit multiply-adds otherwise sit in every stage, ahead of its MFMAs)
  const float* prow[4];    // row kinds: row j at k = tb (ROWS_CAT: first source)
  const float* prow1[4];   // ROWS_CAT: row j of the second source at k = tb
  const float* pcol;       // COLS: k = ta, first of the thread's 4 rows

  __device__ __forceinline__ void init(const fx_operand& op, const float* p0, int r0_, int R_, int K_, int tid,
                                       const SeqOff& soff_, int nsoff_) {
    o = op;
    base = p0;
    nsoff = (KIND == ROWS_CONV || KIND == ROWS_GEN || KIND == COLS_CONVR) ? nsoff_ : 0;
    if (KIND == ROWS_GEN || KIND == COLS_CONVR) {   // the generic element fetch (edge shapes) looks rows up per element
#pragma unroll
      for (int i = 0; i <= kMaxSeq; ++i) soff[i] = soff_[i];
    }
    R = R_;
    K = K_;
    r0 = r0_;
    if (KW == 32 && kRowImg) {
      ta = tid >> 3;
      tb = (tid & 7) * 4;
    } else {
      ta = tid >> 4;
      tb = (tid & 15) * 4;
    }
    if (!FAST) return;
    if (kRowImg) {
      rok = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int r = r0 + ta + RSTEP * j;
        rok |= (r < R ? 1u : 0u) << j;
        rowc[j] = min(r, R - 1);
        if (KIND == ROWS_CONV) seq_pos(op.seq_len, soff_, nsoff_, rowc[j], rmod[j], rlen[j]);
        if (KIND == ROWS_CAT) {
          const int rr = rowc[j];
          rowc1[j] = op.rows1 ? op.rows1[rr] : rr;
          rowc[j] = op.rows0 ? op.rows0[rr] : rr;
        }
        prow[j] = p0 + (long long)rowc[j] * op.ld + tb;
        if (KIND == ROWS_CAT) prow1[j] = op.ptr1 ? op.ptr1 + (long long)rowc1[j] * op.ld1 + tb : prow[j];
      }
    } else {
      // rows that exist in storage: all but a trailing virtual ones row
      const int stored = op.ones_col ? op.ones_col - 1 : R;
      const int r = r0 + tb;
      emask = omask = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        emask |= (r + e < stored ? 1u : 0u) << e;
        omask |= (op.ones_col && r + e == op.ones_col - 1 ? 1u : 0u) << e;
      }
      rc = min(r, ((stored - 1) / 4) * 4);
      pcol = p0 + (long long)ta * op.ld + rc;
      if (KIND == COLS_CONV || KIND == COLS_CONVR) {
        const int j = rc / op.conv_cin;
        tapc = rc - j * op.conv_cin;
        tap_s = conv_shift(op, j);
      }
    }
  }

  // Loads are raw and unconditional; every validity select is applied when the registers are
  // written to LDS (store), a full stage later -- a select right after the load would make the
  // compiler wait for the load there and serialise the prefetch.
  // vm: per-stage validity bits (row-major: bit j = row j valid; COLS_CONV: bit j = time in range)
  __device__ __forceinline__ void load(int k0, float4* v, unsigned& vm) const {
    if (!FAST) {
      load_generic(k0, v);
      vm = 0xFu;
      return;
    }
    if (KIND == ROWS) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = ldg4(prow[j] + k0);
      vm = rok;
    } else if (KIND == ROWS_CONV) {
      // the 64-deep stage lies in one tap (conv_cin % 64 == 0, checked on the host): a uniform
      // channel offset and a uniform row shift, taken per row only where the shifted frame exists
      const int tap = k0 / o.conv_cin;
      const int c = k0 - tap * o.conv_cin;
      const int s = conv_shift(o, tap);
      const long long soff = (long long)s * o.ld;
      vm = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int t = rmod[j] + s;
        const bool ok = ((rok >> j) & 1u) && t >= 0 && t < rlen[j];
        vm |= (ok ? 1u : 0u) << j;
        v[j] = ldg4(prow[j] + c + (ok ? soff : 0ll));
      }
    } else if (KIND == ROWS_CAT) {
      // the whole stage reads one source (k_split % 64 == 0): a uniform choice of row addresses
      const bool second = o.ptr1 && k0 >= o.k_split;
      const int kk = second ? k0 - o.k_split : k0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = ldg4((second ? prow1[j] : prow[j]) + kk);
      vm = rok;
    } else if (KIND == COLS) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) v[j] = ldg4(pcol + (long long)(k0 + RSTEP * j) * o.ld);
      vm = 0xFu;
    } else if (KIND == COLS_KT) {
      vm = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = k0 + ta + RSTEP * j;
        const bool ok = k < K;
        vm |= (ok ? 1u : 0u) << j;
        v[j] = ldg4(pcol + (long long)((ok ? k : K - 1) - ta) * o.ld);
      }
    } else if (KIND == COLS_CONV) {
      vm = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = k0 + ta + RSTEP * j;
        const int t = k % o.seq_len + tap_s;   // (uniform videos only: ragged weight gradients run per video)
        const bool ok = t >= 0 && t < o.seq_len;
        vm |= (ok ? 1u : 0u) << j;
        v[j] = ldg4(base + (long long)(ok ? k + tap_s : k) * o.ld + tapc);
      }
    } else if (KIND == COLS_CONVR) {
      vm = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = k0 + ta + RSTEP * j;
        const bool ok = seq_same(soff, k, tap_s);
        vm |= (ok ? 1u : 0u) << j;
        v[j] = ldg4(base + (long long)(ok ? k + tap_s : k) * o.ld + tapc);
      }
    }
  }

  __device__ __forceinline__ void load_generic(int k0, float4* v) const {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float e[4];
      if (kRowImg) {
        const int r = r0 + ta + RSTEP * j;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0 + tb + q;
          e[q] = (r < R && k < K) ? fetch_rm(o, base, r, k, soff, nsoff) : 0.f;
        }
      } else {
        const int k = k0 + ta + RSTEP * j;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = r0 + tb + q;
          e[q] = (r < R && k < K) ? fetch_cm(o, base, r, k) : 0.f;
        }
      }
      v[j] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }

  __device__ __forceinline__ void store(float* img, const float4* v, unsigned vm) const {
    if (kRowImg) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 x = (!FAST || ((vm >> j) & 1u)) ? v[j] : zero4();
        *reinterpret_cast<float4*>(img + (ta + RSTEP * j) * RS + tb) = x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        if (FAST) {
          const bool tok = (KIND != COLS_CONV && KIND != COLS_CONVR && KIND != COLS_KT) || ((vm >> j) & 1u);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // (COLS_KT: rows past K are zero, the ones row included)
            const float one = (((omask >> q) & 1u) && (KIND != COLS_KT || tok)) ? 1.f : 0.f;
            e[q] = (tok && ((emask >> q) & 1u)) ? e[q] : one;
          }
        }
        float* d = img + (ta + RSTEP * j) * CS + tb;
        d[0] = e[0]; d[1] = e[1]; d[2] = e[2]; d[3] = e[3];
      }
    }
  }

  // MFMA operand of steps 4q..4q+3 for lane (i = row in the wave's 32-row half at wr, h = k half)
  __device__ __forceinline__ static float4 frag(const float* img, int wr, int i, int h, int q) {
    if (kRowImg) return *reinterpret_cast<const float4*>(img + (wr + i) * RS + h * 32 + 4 * q);
    const float* p = img + (h * 32 + 4 * q) * CS + wr + i;
    return make_float4(p[0], p[CS], p[2 * CS], p[3 * CS]);
  }
};

// epilogue: v = alpha*acc (+bias) [relu==2: ReLU here] (+resid) (+beta*C_old) (*gate>0) [relu==1: ReLU]
// c_tap_cin != 0: output column n = tap*c_tap_cin + c is stored at c*3 + tap (Conv1d weight layout)
// c_last != NULL: output column N-1 goes to c_last[m] (fused bias gradient)
__device__ __forceinline__ float* epilogue_ptr(const GemmDev& g, int b, int m, int n) {
  if (g.c_last && n == g.N - 1) return g.c_last + (long long)b * g.c_last_bs + m;
  long long col = n;
  if (g.c_tap_cin) {
    const int j = n / g.c_tap_cin;
    col = (long long)(n - j * g.c_tap_cin) * 3 + j;
  }
  return g.c + (long long)b * g.c_bs + (long long)m * g.ldc + col;
}

// `pre`: the caller has already loaded the old C value into `cold` (beta != 0), else it is read here
__device__ __forceinline__ void epilogue_store(const GemmDev& g, int b, int m, int n, float acc, bool pre = false,
                                               float cold = 0.f) {
  float v = g.alpha * acc;
  float* cp = epilogue_ptr(g, b, m, n);
  if (g.c_last && n == g.N - 1) {
    if (g.beta != 0.f) v += g.beta * (pre ? cold : *cp);
    *cp = v;
    return;
  }
  if (g.bias) v += g.bias[(long long)b * g.bias_bs + n];
  if (g.relu == 2) v = fmaxf(v, 0.f);
  if (g.drop_thr) {
    const unsigned long long idx = ((unsigned long long)b * g.M + m) * g.N + n;
    v = fx_drop_bits(g.drop_seed, idx) >= g.drop_thr ? v * g.drop_scale : 0.f;
  }
  if (g.resid) v += g.resid[(long long)b * g.resid_bs + (long long)m * g.ld_resid + n];
  if (g.beta != 0.f) v += g.beta * (pre ? cold : *cp);
  if (g.gate && !(g.gate[(long long)m * g.ld_gate + n] > 0.f)) v = 0.f;
  if (g.relu == 1) v = fmaxf(v, 0.f);
  *cp = v;
}

// split-K without a second launch: each block of a tile writes its partial sums to its
// workspace slab; the last block to arrive (per-tile counter) adds the slabs in slab order
// (deterministic) and runs the epilogue, then re-arms the counter for the next launch.
// Ordering follows the agent-scope hand-off recipe (cdna_hip_programming.md, projection GEMM
// item 2): drain the slab stores, ONE release fence by lane 0 before the ticket, ONE acquire fence
// in the reducer; correct for any placement of a tile's slices over XCDs.  `flag` lives inside the
// kernel's existing LDS array (a separate __shared__ word can de-pipeline the k-loop).
template <int TM, int TN>
__device__ void splitk_finish(const GemmDev& g, int bidx, int m0, int n0, int tile_id, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev =
        __hip_atomic_fetch_add(&g.tile_cnt[tile_id], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == (unsigned)g.split - 1;
    if (last) {
      __hip_atomic_store(&g.tile_cnt[tile_id], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  if (!*flag) return;
  const long long MN = (long long)g.M * g.N;
  const float* base = g.ws + (long long)bidx * g.split * MN;
  for (int e = threadIdx.x; e < TM * TN; e += blockDim.x) {
    const int m = m0 + e / TN, n = n0 + e % TN;
    if (m >= g.M || n >= g.N) continue;
    const float* p = base + (long long)m * g.N + n;
    float v = 0.f;
    for (int k = 0; k < g.split; ++k) v += p[k * MN];
    epilogue_store(g, bidx, m, n, v);
  }
}
// Output tile (tx, ty) and z-plane (batch x split-K slice) of this block.  Workgroups go to the 8 XCDs
// round robin by linear dispatch id.  Default: within each z-plane, runs of consecutive tiles (one
// row band's column tiles) share an XCD and its L2.  xcd_planes (launches whose plane count is a
// multiple of 8, e.g. the batched / split weight-gradient GEMMs, K = 8192 rows): plane p runs whole
// on XCD p % 8, so every tile reading the plane's A rows and B rows hits one L2 instead of all eight
// XCDs fetching them from MALL / HBM.
__device__ __forceinline__ void block_tile_id(const GemmDev& g, int id, int& tx, int& ty);
__device__ __forceinline__ void block_tile(const GemmDev& g, int& tx, int& ty, int& z) {
  const int nt = g.tiles_x * g.tiles_y;
  if (g.xcd_planes) {
    const int L = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int x8 = L & 7, sl = L >> 3;
    const int pl = sl / nt, t = sl - pl * nt;
    z = pl * 8 + x8;
    ty = t / g.tiles_x;
    tx = t - ty * g.tiles_x;
    return;
  }
  block_tile_id(g, blockIdx.y * g.tiles_x + blockIdx.x, tx, ty);
  z = blockIdx.z;
}
// the (x, y) tile of linear workgroup id `id` (XCD id % 8): XCD runs, then the group / row-permutation orders
__device__ __forceinline__ void block_tile_id(const GemmDev& g, int id, int& tx, int& ty) {
  const int nt = g.tiles_x * g.tiles_y;
  const int q = nt / 8, rr = nt % 8, x8 = id % 8, i8 = id / 8;
  const int nid = (x8 < rr ? x8 * (q + 1) : rr * (q + 1) + (x8 - rr) * q) + i8;
  ty = nid / g.tiles_x;
  tx = nid - ty * g.tiles_x;
  if (g.group_m > 1) {
    // a large B: in row-major order the 32 tiles an XCD runs at once span one row tile and every column
    // tile, so each row tile re-streams all of B through the XCD's L2.  Groups of group_m row tiles (one
    // XCD run), walked column by column: the tiles in flight share a few B columns and the group's A rows
    // (both L2-resident), so B is fetched about once per XCD
    const int gsz = g.group_m * g.tiles_x, grp = nid / gsz, r = nid - grp * gsz;
    const int rows = min(g.group_m, g.tiles_y - grp * g.group_m);
    ty = grp * g.group_m + r % rows;
    tx = r / rows;
  }
  if (g.row_perm > 1) {
    // a dilated conv whose taps shift by row_perm whole row tiles: the XCD runs walk the row tiles in
    // the order 0, p, 2p, ..., 1, 1 + p, ... so the tiles holding a tile's shifted rows sit next to it in
    // its run (same L2) instead of one or more runs away (HBM / MALL re-reads)
    const int per = g.tiles_y / g.row_perm;
    ty = (ty % per) * g.row_perm + ty / per;
  }
}

__device__ __forceinline__ void tile_epilogue(const GemmDev& g, int bidx, int rbase, int col, const f32x16& acc) {
  if (col >= g.N) return;
  if (!g.c_last && !g.c_tap_cin && !g.gate && g.beta == 0.f && !g.drop_thr) {
    const float bv = g.bias ? g.bias[(long long)bidx * g.bias_bs + col] : 0.f;
    float res[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      res[r] = (g.resid && row < g.M) ? g.resid[(long long)bidx * g.resid_bs + (long long)row * g.ld_resid + col]
                                      : 0.f;
    }
    float* cb = g.c + (long long)bidx * g.c_bs + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      float v = g.alpha * acc[r] + bv;
      if (g.relu == 2) v = fmaxf(v, 0.f);
      v += res[r];
      if (g.relu == 1) v = fmaxf(v, 0.f);
      if (row < g.M) cb[(long long)row * g.ldc] = v;   // (non-temporal stores measured even: round 2)
    }
  } else {   // (a preloaded-C variant here costs the 128x64 kernel 416 B of scratch)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + (r & 3) + 8 * (r >> 2);
      if (row < g.M) epilogue_store(g, bidx, row, col, acc[r]);
    }
  }
}

}  // namespace

// The members of one grouped direct launch (gemm_direct.hip)
constexpr int GMAX = 4;
struct GemmGroup {
  GemmDev g[GMAX];
  int kinds[GMAX];         // ak * 8 + bk
  int start[GMAX + 1];     // first flat block of each problem
  int n;
};

}  // namespace fx
