// One MS-TCN++ layer step as ONE kernel (MSTCN2.forward, basic.py:271-277, and the matching input-gradient
// chain), on the tile geometry and operand paths of the fused MS-TCN layer (mstcn_fused.hip, frl_dev.h): a
// workgroup owns FR = 32 rows and all F = 256 channels, the activation rows of a stage go through the paired
// LDS ring, every wave loads its own weight fragments PD stages ahead from matrices in the packed order of
// launch_pack_frag, and the intermediate tile V stays in LDS.  No workgroup talks to another.
//
//   forward  (layer i):  A = conv_d1,i(f_i) + b_d1 -> cat_i[:, 0:F], V[:, 0:F]      (K = 3F, dilation dil[0])
//                        B = conv_d2,i(f_i) + b_d2 -> cat_i[:, F:2F], V[:, F:2F]    (K = 3F, dilation dil[1])
//                        r_i = dropout_i(relu(V . W_fu^T + b_fu)) -> out2           (K = 2F from LDS)
//                        f_i+1 = f_i + r_i -> out3
//   backward (chain step i, G_i the gradient at f_i):
//                        G_i = G_i+1 + conv_d1,i^T(dCat_i[:, 0:F]) + conv_d2,i^T(dCat_i[:, F:2F]) -> out1
//                                                                   (ONE accumulator over K = 2 . 3F)
//                        dU_i-1 = dropout_i-1(G_i) * (r_i-1 > 0) -> outv, V
//                        dCat_i-1 = dU_i-1 . W_fu,i-1 -> out2 (ld 2F)   (two 256-column passes, K = F from LDS)
//
// Phase 1 is 48 stages in both modes: stages 0..23 are conv_d1's taps, 24..47 conv_d2's, each with its own
// tap shift, weight matrix and operand column offset (forward: both read f_i; backward: the halves of dCat_i).
// The forward empties the accumulator into V between the two; the backward keeps summing.  Phase 2 is 16
// stages in both modes (forward: one K = 512 product; backward: two K = 256 products on the same V rows).
#include <algorithm>

#include "frl_dev.h"
#include "fx_common.h"
#include "ops.h"

namespace fx {
namespace {

using namespace frl_dev;

constexpr int NS1 = 3 * FN / FBK;         // stages of one dilated conv (K = 3F)
constexpr int NP1 = 2 * NS1;              // phase 1: both convs
constexpr int NS2 = 2 * FN / FBK;         // phase 2
constexpr int RING = 2 * NSL * A_IMG;     // the paired activation ring
constexpr int VS_FWD = 2 * FN + 4;        // LDS row stride of V: [A | B] forward, dU backward
constexpr int VS_BWD = FN + 4;
constexpr int LDS_FWD = RING + FR * VS_FWD;   // 93.7 KB: one workgroup per CU, as frl_kernel
constexpr int LDS_BWD = RING + FR * VS_BWD;

struct Frl2Args {
  const float* x;        // phase-1 operand rows, ld ldx; conv h reads columns h * xcol .. + FN
  long long ldx;
  int xcol;              // 0 forward (both convs read f_i), FN backward (the halves of dCat_i)
  int dil[2], dir, T, M;
  int xcd_runs;          // consecutive row tiles share an XCD (frl_tile_id)
  int nsoff;             // > 0: ragged videos, video v owns rows [soff[v], soff[v+1])
  int soff[kMaxSeqF + 1];
  const float* w1[2];    // packed conv weights of conv_d1 / conv_d2 (forward or dX orientation), K = 3 FN
  const float* bias1[2]; // forward: b_d1, b_d2
  float* out1;           // forward: cat_i (conv h at column h * FN); backward: G_i
  long long ldo1;
  const float* resid1;   // backward: G_i+1
  long long ldr1;
  const float* gate;     // backward: r_i-1 (dU is zero where it is not positive)
  long long ldg;
  float* outv;           // backward: the dU_i-1 slot
  long long ldov;
  const float* w2;       // forward: packed W_fu (K = 2 FN); backward: packed W_fu^T halves, half h at h * FN * FN
  const float* bias2;    // forward: b_fu
  const float* resid2;   // forward: f_i
  long long ldr2;
  float* out2;           // forward: r_i; backward: dCat_i-1 (half h at column h * FN)
  long long ldo2;
  float* out3;           // forward: f_i+1
  long long ldo3;
  unsigned drop_thr;     // forward: dropout_i on relu(u); backward: dropout_i-1 on G_i as dU reads it; 0 = off
  float drop_scale;
  unsigned long long drop_seed;
};

template <bool BWD, int PD>
__global__ __launch_bounds__(FT) void frl2_kernel(Frl2Args g) {
  constexpr int NB = PD + 1;
  constexpr int VS = BWD ? VS_BWD : VS_FWD;
  constexpr int nall = NP1 + NS2, np = NP1 / 2;
  static_assert(NS1 % 2 == 0 && NP1 % NB == 0, "stage pairs; register sets line up across the phases");
  extern __shared__ float lds[];
  float* V = lds + RING;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int m0 = frl_tile_id(g.xcd_runs, 1) * FR;
  // this thread's activation row and its position inside its video; threads 0..255 stage the even stage of
  // a pair, 256..511 the odd one
  const int ar = (tid & 255) >> 3, k4 = (tid & 7) * 4, half = tid >> 8;
  const int r = m0 + ar;
  int rpos, rlen;
  frl_row_pos(r, g.nsoff, g.soff, g.T, rpos, rlen);
  const bool rok = r < g.M;
  const float* xrow = g.x + (long long)min(r, g.M - 1) * g.ldx + k4;
  // stage 2 pr + half: conv h = pr / 12, its tap and channel block
  auto load_a = [&](int pr, float4& v, bool& ok) {
    const int h = pr / (NS1 / 2), s2 = 2 * (pr - h * (NS1 / 2)) + half;
    const int k0 = s2 * FBK, tap = k0 / FN, c0 = k0 - tap * FN;
    const int sh = (tap - 1) * g.dil[h] * g.dir;
    const int t = rpos + sh;
    ok = rok && t >= 0 && t < rlen;
    v = ld4(xrow + (ok ? (long long)sh * g.ldx : 0ll) + c0 + h * g.xcol);   // clamped, unconditional load
  };
  auto store_a = [&](float* slot, const float4& v, bool ok) {
    st4(slot + ar * AS + k4, ok ? v : make_float4(0.f, 0.f, 0.f, 0.f));
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float4 pb[NB][4];                    // weight fragments, register set st % NB
  float4 pa;                           // this thread's activation row, two pairs ahead
  bool pok;
  auto load_w = [&](int st) {
    if (st < NS1) load_b(g.w1[0], st, w, lane, pb[st % NB]);
    else if (st < NP1) load_b(g.w1[1], st - NS1, w, lane, pb[st % NB]);
    else if (st < nall) {
      const int j = st - NP1;
      if constexpr (BWD) load_b(g.w2 + (long long)(j / (NS2 / 2)) * FN * FN, j % (NS2 / 2), w, lane, pb[st % NB]);
      else load_b(g.w2, j, w, lane, pb[st % NB]);
    }
  };
  const int ecol = w * 32 + li;
  auto erow = [&](int q) { return (q & 3) + 8 * (q >> 2) + 4 * lh; };   // accumulator element q's tile row
  auto grow = [&](int q) { return min(m0 + erow(q), g.M - 1); };
  // backward epilogue operands, loaded before the MFMAs they follow
  float r1[16], gat[16];
  auto load_r1 = [&]() {
    if constexpr (BWD) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        r1[q] = g.resid1[(long long)grow(q) * g.ldr1 + ecol];
        gat[q] = g.gate[(long long)grow(q) * g.ldg + ecol];
      }
    }
  };
  // forward: conv h's tile (+ bias) to its half of cat_i and of V; the accumulator starts over
  auto store_cat = [&](int h) {
    const float bv = g.bias1[h][ecol];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = erow(q), gr = m0 + row;
      const float v = acc[q] + bv;
      if (gr < g.M) g.out1[(long long)gr * g.ldo1 + h * FN + ecol] = v;
      V[row * VS + h * FN + ecol] = v;
      acc[q] = 0.f;
    }
  };
#pragma unroll
  for (int st = 0; st < PD; ++st) load_w(st);
  auto slot = [&](int p) { return lds + (p % NSL) * 2 * A_IMG; };
  {
    float4 p1;
    bool ok1;
    load_a(0, pa, pok);
    load_a(1, p1, ok1);
    store_a(slot(0) + half * A_IMG, pa, pok);
    store_a(slot(1) + half * A_IMG, p1, ok1);
    load_a(2, pa, pok);
  }
  __syncthreads();
  // A fragments of pair p are read from LDS one pair ahead (during pair p - 1's MFMAs): slot p % NSL was
  // written before the barrier that ended pair p - 2, so the read needs no extra barrier
  float4 fa[2][2][4];   // [pair parity][stage of the pair][q]
  lds_frag(slot(0), AS, li, lh, fa[0][0]);
  lds_frag(slot(0) + A_IMG, AS, li, lh, fa[0][1]);
#pragma unroll
  for (int p = 0; p < np; ++p) {
    if (p + 1 < np) {
      lds_frag(slot(p + 1), AS, li, lh, fa[(p + 1) & 1][0]);
      lds_frag(slot(p + 1) + A_IMG, AS, li, lh, fa[(p + 1) & 1][1]);
    } else {
      load_r1();
    }
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(fa[p & 1][0], pb[(2 * p) % NB], acc);
    __builtin_amdgcn_sched_barrier(0);
    load_w(2 * p + PD);
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(fa[p & 1][1], pb[(2 * p + 1) % NB], acc);
    __builtin_amdgcn_sched_barrier(0);
    // pair p + 2 (loaded during the previous pair) into the slot pair p - 1 used (its fragments were read
    // during pair p - 2); fetch pair p + 3
    if (p + 2 < np) store_a(slot(p + 2) + half * A_IMG, pa, pok);
    if (p + 3 < np) load_a(p + 3, pa, pok);
    load_w(2 * p + 1 + PD);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!BWD)
      if (p == np / 2 - 1) store_cat(0);   // (V is read only after the barrier that ends phase 1)
    __syncthreads();
  }
  // ---------------- phase-1 epilogue: the rest of V
  float res[16];
  if constexpr (BWD) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = erow(q), gr = m0 + row;
      float v = acc[q] + r1[q];
      if (gr < g.M) g.out1[(long long)gr * g.ldo1 + ecol] = v;
      if (g.drop_thr)
        v = fx_drop_bits(g.drop_seed, (unsigned long long)gr * FN + ecol) >= g.drop_thr ? v * g.drop_scale : 0.f;
      if (!(gat[q] > 0.f)) v = 0.f;
      if (gr < g.M) g.outv[(long long)gr * g.ldov + ecol] = v;
      V[row * VS + ecol] = v;
      acc[q] = 0.f;
    }
  } else {
    store_cat(1);
#pragma unroll
    for (int q = 0; q < 16; ++q) res[q] = g.resid2[(long long)grow(q) * g.ldr2 + ecol];
  }
  __syncthreads();
  // ---------------- phase 2 from the LDS tile, no barrier: V fragments one stage ahead
  float4 fv[2][4];
  auto vstage = [&](int j) { return V + (BWD ? j % (NS2 / 2) : j) * FBK; };
  lds_frag(vstage(0), VS, li, lh, fv[0]);
#pragma unroll
  for (int j = 0; j < NS2; ++j) {
    if (j + 1 < NS2) lds_frag(vstage(j + 1), VS, li, lh, fv[(j + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    mma_frag(fv[j & 1], pb[(NP1 + j) % NB], acc);
    __builtin_amdgcn_sched_barrier(0);
    load_w(NP1 + j + PD);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (BWD) {
      if (j % (NS2 / 2) == NS2 / 2 - 1) {   // dCat_i-1's half h = dU . W_fu[:, h F ..]
        const int h = j / (NS2 / 2);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int gr = m0 + erow(q);
          if (gr < g.M) g.out2[(long long)gr * g.ldo2 + h * FN + ecol] = acc[q];
          acc[q] = 0.f;
        }
      }
    }
  }
  if constexpr (!BWD) {   // r_i = dropout_i(relu(u)), f_i+1 = f_i + r_i
    const float bv = g.bias2[ecol];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int gr = m0 + erow(q);
      float v = fmaxf(acc[q] + bv, 0.f);
      if (g.drop_thr)
        v = fx_drop_bits(g.drop_seed, (unsigned long long)gr * FN + ecol) >= g.drop_thr ? v * g.drop_scale : 0.f;
      if (gr < g.M) {
        g.out2[(long long)gr * g.ldo2 + ecol] = v;
        g.out3[(long long)gr * g.ldo3 + ecol] = res[q] + v;
      }
    }
  }
}

int frl2_common(Frl2Args& a, const Frl2Layer& y) {
  FX_REQUIRE(y.M > 0 && y.dil1 > 0 && y.dil2 > 0, "frl2: bad shape");
  FX_REQUIRE(y.seq_off ? (y.nseq >= 1 && y.nseq <= kMaxSeqF && y.seq_off[0] == 0 && y.seq_off[y.nseq] == y.M) : y.T > 0,
             "frl2: uniform videos of T rows, or ragged offsets spanning [0, M) (<= 16 videos)");
  FX_REQUIRE(y.drop_p >= 0.f && y.drop_p < 1.f, "frl2: dropout must be in [0, 1)");
  a.dil[0] = y.dil1;
  a.dil[1] = y.dil2;
  a.T = y.T > 0 ? y.T : 1;
  a.M = y.M;
  a.xcd_runs = knobs().frl_xcd >= 1 && cdiv(y.M, FR) >= 16;
  a.nsoff = y.seq_off ? y.nseq : 0;
  if (y.seq_off)
    for (int v = 0; v <= y.nseq; ++v) a.soff[v] = y.seq_off[v];
  a.drop_thr = y.drop_p > 0.f ? std::max(fx_drop_thresh(y.drop_p), 1u) : 0u;
  a.drop_scale = 1.f / (1.f - y.drop_p);
  a.drop_seed = y.drop_seed;
  static const bool attr = [] {
    return hipFuncSetAttribute((const void*)frl2_kernel<false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               LDS_FWD * (int)sizeof(float)) == hipSuccess &&
           hipFuncSetAttribute((const void*)frl2_kernel<true, 3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               LDS_BWD * (int)sizeof(float)) == hipSuccess;
  }();
  FX_REQUIRE(attr, "frl2: cannot raise the LDS limit");
  return FX_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_frl2_fwd(const Frl2Layer& y, const float* f, const float* w1p, const float* w2p, const float* b1,
                    const float* b2, float* cat, const float* wfup, const float* bfu, float* r, float* fnext,
                    hipStream_t s) {
  FX_REQUIRE(f && w1p && w2p && b1 && b2 && cat && wfup && bfu && r && fnext, "frl2 fwd: null operand");
  FX_REQUIRE(aligned16(f) && aligned16(w1p) && aligned16(w2p) && aligned16(wfup), "frl2: 16-byte aligned operands");
  Frl2Args a{};
  FX_TRY(frl2_common(a, y));
  a.x = f;
  a.ldx = FN;
  a.xcol = 0;
  a.dir = 1;
  a.w1[0] = w1p;
  a.w1[1] = w2p;
  a.bias1[0] = b1;
  a.bias1[1] = b2;
  a.out1 = cat;
  a.ldo1 = 2 * FN;
  a.w2 = wfup;
  a.bias2 = bfu;
  a.resid2 = f;
  a.ldr2 = FN;
  a.out2 = r;
  a.ldo2 = FN;
  a.out3 = fnext;
  a.ldo3 = FN;
  fx_launch((frl2_kernel<false, 3>), dim3(cdiv(y.M, FR)), dim3(FT), LDS_FWD * sizeof(float), s, a);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_frl2_bwd(const Frl2Layer& y, const float* dcat, const float* wb1p, const float* wb2p, const float* gnext,
                    float* gout, const float* rprev, float* du, const float* wfutp, float* dcat_prev, hipStream_t s) {
  FX_REQUIRE(dcat && wb1p && wb2p && gnext && gout && rprev && du && wfutp && dcat_prev, "frl2 bwd: null operand");
  FX_REQUIRE(aligned16(dcat) && aligned16(wb1p) && aligned16(wb2p) && aligned16(wfutp),
             "frl2: 16-byte aligned operands");
  Frl2Args a{};
  FX_TRY(frl2_common(a, y));
  a.x = dcat;
  a.ldx = 2 * FN;
  a.xcol = FN;
  a.dir = -1;
  a.w1[0] = wb1p;
  a.w1[1] = wb2p;
  a.out1 = gout;
  a.ldo1 = FN;
  a.resid1 = gnext;
  a.ldr1 = FN;
  a.gate = rprev;
  a.ldg = FN;
  a.outv = du;
  a.ldov = FN;
  a.w2 = wfutp;
  a.out2 = dcat_prev;
  a.ldo2 = 2 * FN;
  fx_launch((frl2_kernel<true, 3>), dim3(cdiv(y.M, FR)), dim3(FT), LDS_BWD * sizeof(float), s, a);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx
