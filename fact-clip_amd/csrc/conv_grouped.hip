// Grouped dilated Conv1d(k = 3) on CDNA4 matrix cores (nn.Conv1d(F, F, 3, dilation = d, padding = d,
// groups = g): the reference's f_ngp > 1 frame branch).  cg = F / g channels per group; the weight is
// nn.Conv1d's (F, cg, 3): output channel n belongs to group n / cg and its row holds [c][tap].
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact f32 products, fp32 accumulation), whatever the
// stream's GEMM precision mode.  Three kernels:
//
//   gconv_pack_kernel   (F, cg, 3) -> Wf[q][tap][n][c] (forward) and Wb[q][tap][c][n] (dX), both 3 F cg floats
//                       (and, optionally, a 1x1 weight transposed, as the dense pack does)
//   gconv_kernel<NJ>    y[r, q cg + n] = act(sum_tap sum_c x[r + (tap - 1) dil dir, q cg + c] Wp[q][tap][n][c] + b)
//                       (+ resid) (+= y); dir = -1 over Wb is the input gradient.  One launch covers every
//                       group: grid = row tiles x (groups x column tiles).  A workgroup owns 64 rows x
//                       64 NJ columns of ONE group and walks K = 3 cg tap by tap in 32-deep stages through
//                       LDS; 4 waves, each 32 rows x 32 NJ columns (NJ accumulators of 16 VGPRs).
//   gconv_dw_kernel     dWq[n][c][tap] = sum_r dZ[r, q cg + n] x[r + (tap - 1) dil, q cg + c] and
//                       db[n] = sum_r dZ[r, n]: K = rows split over workgroups, each writing its partial
//                       to the workspace; gconv_dw_reduce_kernel sums the partials in split order and
//                       adds them to the caller's (F, cg, 3) / (F) buffers.  No floating-point atomics:
//                       two runs give the same bits.
//
// A shifted row that leaves its video contributes zero (uniform videos of T rows, or up to 16 ragged
// videos by row offsets), and every tile edge is masked: any F % g == 0 is correct, cg a multiple of 4
// (16-byte loads) is the fast loader, cg a multiple of 32 wastes no stage depth.
//
// LDS: images are [row][k] with stride 36 floats (forward; ds_read_b128 fragment reads, conflict-free)
// and [k][col] with stride 68 (weight gradient; b32 reads, the two lane halves 8 k-rows = 32 banks apart).
// Inside a stage a lane half works on its own run of k; both operands agree on the order, which is all
// an MFMA chain needs.  Global loads of stage s + 1 are in flight in registers while stage s multiplies.
#include <algorithm>

#include "ops.h"
#include "wave_dev.h"

namespace fx {
namespace {


constexpr int GBM = 64;        // rows per forward tile
constexpr int GK = 32;         // stage depth
constexpr int GRS = 36;        // forward LDS image stride ([row][k])
constexpr int GCS = 68;        // weight-gradient LDS image stride ([k][col])
constexpr int kGMaxVid = 16;   // ragged videos per call

struct VidMap {
  int T;                    // uniform videos of T rows (nseq == 0)
  int nseq;                 // ragged: videos off[v] .. off[v + 1]
  int off[kGMaxVid + 1];
};

// rows [lo, hi) of the video that owns row r (r < rows)
__device__ __forceinline__ void vid_bounds(const VidMap& v, int r, int rows, int& lo, int& hi) {
  if (v.nseq == 0) {
    lo = (r / v.T) * v.T;
    hi = min(lo + v.T, rows);
  } else {
    lo = 0;
    hi = v.off[1];
#pragma unroll
    for (int i = 1; i < kGMaxVid; ++i)
      if (i < v.nseq && r >= v.off[i]) {
        lo = v.off[i];
        hi = v.off[i + 1];
      }
  }
}

// ---------------------------------------------------------------- pack
constexpr int GPACK_JOBS = 64;
struct GPackArgs {
  const float* w[GPACK_JOBS];
  float* wf[GPACK_JOBS];
  float* wb[GPACK_JOBS];
  const float* wpw[GPACK_JOBS];   // optional 1x1 weight (F, F) -> wpt transposed
  float* wpt[GPACK_JOBS];
  int F, cg;
};

__global__ __launch_bounds__(256) void gconv_pack_kernel(GPackArgs p) {
  const int l = blockIdx.y, F = p.F, cg = p.cg;
  const long long total = 3LL * F * cg;
  const float* w = p.w[l];
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    // e = ((q * 3 + tap) * cg + n) * cg + c   (the forward image's order: coalesced writes)
    const int c = (int)(e % cg);
    long long t = e / cg;
    const int n = (int)(t % cg);
    t /= cg;
    const int tap = (int)(t % 3), q = (int)(t / 3);
    const float v = w[((long long)(q * cg + n) * cg + c) * 3 + tap];
    p.wf[l][e] = v;
    p.wb[l][(((long long)q * 3 + tap) * cg + c) * cg + n] = v;
  }
  if (p.wpt[l]) {
    const long long tt = (long long)F * F;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < tt; e += (long long)gridDim.x * 256) {
      const int c = (int)(e % F), o = (int)(e / F);
      p.wpt[l][(long long)c * F + o] = p.wpw[l][e];
    }
  }
}

// ---------------------------------------------------------------- forward / input gradient
struct GConvArgs {
  const float* x;
  long long ldx;
  const float* wp;      // [q][tap][n][k]
  const float* bias;    // nullable (F)
  const float* resid;   // nullable
  long long ldr;
  float* y;
  long long ldy;
  int rows, cg, ntn, shift;   // shift = dil * dir
  int relu, accumulate, vec;
  VidMap vm;
};

template <int NJ>
__global__ __launch_bounds__(256) void gconv_kernel(GConvArgs a) {
  constexpr int BN = 64 * NJ;
  constexpr int BPT = 8 * NJ;          // B floats per thread per stage
  constexpr int TPR = 4 / NJ;          // B loader threads per weight row
  __shared__ __attribute__((aligned(16))) float As[GBM * GRS];
  __shared__ __attribute__((aligned(16))) float Bs[BN * GRS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int q = blockIdx.y / a.ntn, nt = blockIdx.y - q * a.ntn;
  const int m0 = blockIdx.x * GBM, n0 = nt * BN;
  const int cg = a.cg;
  const int nkc = (cg + GK - 1) / GK, nst = 3 * nkc;

  // loaders: A row tid / 4, 8 k from (tid % 4) * 8; B row tid / TPR, BPT k from (tid % TPR) * BPT
  const int ar = tid >> 2, ak = (tid & 3) * 8;
  const int arow = m0 + ar;
  int lo = 0, hi = 0;   // (a row past the call: empty range, every tap reads zero)
  if (arow < a.rows) vid_bounds(a.vm, arow, a.rows, lo, hi);
  const int br = tid / TPR, bk = (tid % TPR) * BPT;
  const int bn = n0 + br;

  float ra[8], rb[BPT];
  auto load_stage = [&](int s) {
    const int tap = s / nkc, c0 = (s - tap * nkc) * GK;
    const int rs = arow + (tap - 1) * a.shift;
    const bool rv = rs >= lo && rs < hi;
    const float* px = a.x + (long long)rs * a.ldx + (long long)q * cg + c0 + ak;
    const float* pw = a.wp + (((long long)q * 3 + tap) * cg + bn) * cg + c0 + bk;
    if (a.vec) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rv && c0 + ak + 4 * j < cg) v = *reinterpret_cast<const float4*>(px + 4 * j);
        ra[4 * j] = v.x, ra[4 * j + 1] = v.y, ra[4 * j + 2] = v.z, ra[4 * j + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < BPT / 4; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bn < cg && c0 + bk + 4 * j < cg) v = *reinterpret_cast<const float4*>(pw + 4 * j);
        rb[4 * j] = v.x, rb[4 * j + 1] = v.y, rb[4 * j + 2] = v.z, rb[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) ra[j] = (rv && c0 + ak + j < cg) ? px[j] : 0.f;
#pragma unroll
      for (int j = 0; j < BPT; ++j) rb[j] = (bn < cg && c0 + bk + j < cg) ? pw[j] : 0.f;
    }
  };

  f32x16 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  const int wr = (w & 1) * 32, wc = (w >> 1) * 32 * NJ;
  load_stage(0);
  for (int s = 0; s < nst; ++s) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      *reinterpret_cast<float4*>(&As[ar * GRS + ak + 4 * j]) =
          make_float4(ra[4 * j], ra[4 * j + 1], ra[4 * j + 2], ra[4 * j + 3]);
#pragma unroll
    for (int j = 0; j < BPT / 4; ++j)
      *reinterpret_cast<float4*>(&Bs[br * GRS + bk + 4 * j]) =
          make_float4(rb[4 * j], rb[4 * j + 1], rb[4 * j + 2], rb[4 * j + 3]);
    __syncthreads();
    if (s + 1 < nst) load_stage(s + 1);
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
      const float4 fa = *reinterpret_cast<const float4*>(&As[(wr + li) * GRS + 16 * lh + 4 * j4]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 fb = *reinterpret_cast<const float4*>(&Bs[(wc + j * 32 + li) * GRS + 16 * lh + 4 * j4]);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // epilogue: bias, ReLU, residual, accumulate; accumulator r of a lane is row (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cl = n0 + wc + j * 32 + li;   // column inside the group
    if (cl >= cg) continue;
    const long long col = (long long)q * cg + cl;
    const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row >= a.rows) continue;
      float v = acc[j][r] + bv;
      if (a.relu) v = fmaxf(v, 0.f);
      if (a.resid) v += a.resid[(long long)row * a.ldr + col];
      float* py = a.y + (long long)row * a.ldy + col;
      if (a.accumulate) v += *py;
      *py = v;
    }
  }
}

// ---------------------------------------------------------------- weight / bias gradient
struct GDwArgs {
  const float* dz;
  long long lddz;
  const float* x;
  long long ldx;
  float* part;     // [split][F][3][cg]
  float* dbpart;   // [split][F]
  int rows, cg, F, ntc, dil, rows_per_split, vec;
  VidMap vm;
};

__global__ __launch_bounds__(256) void gconv_dw_kernel(GDwArgs a) {
  __shared__ __attribute__((aligned(16))) float Zs[GK * GCS];
  __shared__ __attribute__((aligned(16))) float Xs[3][GK * GCS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int cg = a.cg, ntc = a.ntc;
  const int q = blockIdx.x / (ntc * ntc);
  const int tt = blockIdx.x - q * ntc * ntc;
  const int tn = tt / ntc, tc = tt - tn * ntc;
  const int sk = blockIdx.y;
  const int k0 = sk * a.rows_per_split, k1 = min(a.rows, k0 + a.rows_per_split);
  const int nst = k1 > k0 ? (k1 - k0 + GK - 1) / GK : 0;

  // loader: row tid / 8 of the stage, 8 columns from (tid % 8) * 8, of each of the four images
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int zc = tn * 64 + lc, xc = tc * 64 + lc;   // columns inside the group
  float rz[8], rx[3][8];
  auto load_stage = [&](int s) {
    const int r = k0 + s * GK + lr;
    const bool rv = r < k1;
    int lo = 0, hi = 0;
    if (rv) vid_bounds(a.vm, r, a.rows, lo, hi);
    const float* pz = a.dz + (long long)r * a.lddz + (long long)q * cg + zc;
    if (a.vec) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rv && zc + 4 * j < cg) v = *reinterpret_cast<const float4*>(pz + 4 * j);
        rz[4 * j] = v.x, rz[4 * j + 1] = v.y, rz[4 * j + 2] = v.z, rz[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) rz[j] = (rv && zc + j < cg) ? pz[j] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int rs = r + (t - 1) * a.dil;
      const bool tv = rs >= lo && rs < hi;
      const float* px = a.x + (long long)rs * a.ldx + (long long)q * cg + xc;
      if (a.vec) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (tv && xc + 4 * j < cg) v = *reinterpret_cast<const float4*>(px + 4 * j);
          rx[t][4 * j] = v.x, rx[t][4 * j + 1] = v.y, rx[t][4 * j + 2] = v.z, rx[t][4 * j + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) rx[t][j] = (tv && xc + j < cg) ? px[j] : 0.f;
      }
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  float dbacc = 0.f;
  const int nh = (w & 1) * 32, ch = (w >> 1) * 32;
  const bool do_db = a.dbpart && tc == 0 && tid < 64;

  if (nst > 0) load_stage(0);
  for (int s = 0; s < nst; ++s) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<float4*>(&Zs[lr * GCS + lc + 4 * j]) =
          make_float4(rz[4 * j], rz[4 * j + 1], rz[4 * j + 2], rz[4 * j + 3]);
#pragma unroll
      for (int t = 0; t < 3; ++t)
        *reinterpret_cast<float4*>(&Xs[t][lr * GCS + lc + 4 * j]) =
            make_float4(rx[t][4 * j], rx[t][4 * j + 1], rx[t][4 * j + 2], rx[t][4 * j + 3]);
    }
    __syncthreads();
    if (s + 1 < nst) load_stage(s + 1);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const int kr = (ks & 7) + 16 * (ks >> 3) + 8 * lh;   // the lane halves 8 k-rows apart: 32 banks
      const float av = Zs[kr * GCS + nh + li];
#pragma unroll
      for (int t = 0; t < 3; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Xs[t][kr * GCS + ch + li], acc[t], 0, 0, 0);
    }
    if (do_db) {   // bias gradient of this tile's 64 output channels: fixed row order
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < GK; ++k) v += Zs[k * GCS + tid];
      dbacc += v;
    }
    __syncthreads();
  }

#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int cl = tc * 64 + ch + li;
    if (cl >= cg) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int nl = tn * 64 + nh + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (nl >= cg) continue;
      a.part[(((long long)sk * a.F + (long long)q * cg + nl) * 3 + t) * cg + cl] = acc[t][r];
    }
  }
  if (do_db && tn * 64 + tid < cg) a.dbpart[(long long)sk * a.F + (long long)q * cg + tn * 64 + tid] = dbacc;
}

// dw[(n, c, tap)] += sum over the splits, in split order; db likewise
__global__ __launch_bounds__(256) void gconv_dw_reduce_kernel(const float* part, const float* dbpart, int nsplit,
                                                              int F, int cg, float* dw, float* db) {
  const long long nw = 3LL * F * cg;
  const long long total = nw + (db ? F : 0);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    float v = 0.f;
    if (e < nw) {
      if (!dw) continue;
      for (int s = 0; s < nsplit; ++s) v += part[s * nw + e];
      const int c = (int)(e % cg);
      const long long t = e / cg;
      const int tap = (int)(t % 3);
      const long long n = t / 3;
      dw[(n * cg + c) * 3 + tap] += v;
    } else {
      const long long n = e - nw;
      for (int s = 0; s < nsplit; ++s) v += dbpart[(long long)s * F + n];
      db[n] += v;
    }
  }
}

int fill_vidmap(VidMap& vm, int rows, int T, int nvid, const int* seq_off) {
  vm = VidMap{};
  if (seq_off) {
    FX_REQUIRE(nvid >= 1 && nvid <= kGMaxVid && seq_off[0] == 0 && seq_off[nvid] == rows,
               "grouped conv: ragged offsets start at 0, end at rows, <= 16 videos");
    for (int v = 0; v < nvid; ++v) FX_REQUIRE(seq_off[v + 1] > seq_off[v], "grouped conv: empty video");
    vm.nseq = nvid;
    for (int v = 0; v <= nvid; ++v) vm.off[v] = seq_off[v];
    for (int v = nvid + 1; v <= kGMaxVid; ++v) vm.off[v] = rows;
  } else {
    FX_REQUIRE(T >= 1 && nvid >= 1 && (long long)T * nvid == rows, "grouped conv: rows must be T * nvid");
    vm.T = T;
  }
  return FX_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void dw_split(int rows, int F, int ngroup, int& nsplit, int& rps) {
  const int cg = F / ngroup, ntc = cdiv(cg, 64);
  const long long tiles = (long long)ngroup * ntc * ntc;
  const int want = (int)std::max<long long>(1, std::min<long long>(32, 512 / tiles));
  const int n0 = std::max(1, std::min(want, cdiv(rows, 128)));
  rps = cdiv(cdiv(std::max(rows, 1), n0), GK) * GK;
  nsplit = std::max(1, cdiv(rows, rps));
}

}  // namespace

int gconv_check(int F, int ngroup, const char* who) {
  if (ngroup < 0 || F < 1 || F % std::max(ngroup, 1) != 0) {
    set_error(std::string(who) + ": ngroup must be >= 0 and divide F");
    return FX_ERR_SHAPE;
  }
  return FX_OK;
}

long long gconv_packed_floats(int F, int ngroup) { return 3LL * F * (F / std::max(ngroup, 1)); }

int launch_gconv_pack(const GPackJob* jobs, int n, int F, int ngroup, hipStream_t s) {
  const int cg = F / ngroup;
  for (int i0 = 0; i0 < n; i0 += GPACK_JOBS) {
    const int nb = std::min(GPACK_JOBS, n - i0);
    GPackArgs a{};
    a.F = F;
    a.cg = cg;
    bool pw = false;
    for (int i = 0; i < nb; ++i) {
      a.w[i] = jobs[i0 + i].w;
      a.wf[i] = jobs[i0 + i].wf;
      a.wb[i] = jobs[i0 + i].wb;
      a.wpw[i] = jobs[i0 + i].wpw;
      a.wpt[i] = jobs[i0 + i].wpt;
      pw = pw || a.wpt[i];
    }
    const long long total = std::max(3LL * F * cg, pw ? (long long)F * F : 0LL);
    fx_launch(gconv_pack_kernel, dim3(ew_grid(total), nb), dim3(256), 0, s, a);
    FX_CHECK_HIP(hipGetLastError());
  }
  return FX_OK;
}

int launch_gconv(const float* x, long long ldx, int rows, int T, int nvid, const int* seq_off, int F, int ngroup,
                 int dil, int dir, const float* wp, const float* bias, int relu, const float* resid, long long ldr,
                 int accumulate, float* y, long long ldy, hipStream_t s) {
  FX_TRY(gconv_check(F, ngroup, "grouped conv"));
  FX_REQUIRE(x && wp && y && rows >= 0 && dil >= 1, "grouped conv: bad arguments");
  if (rows == 0) return FX_OK;
  GConvArgs a{};
  FX_TRY(fill_vidmap(a.vm, rows, T, nvid, seq_off));
  const int g = std::max(ngroup, 1), cg = F / g;
  a.x = x, a.ldx = ldx, a.wp = wp, a.bias = bias, a.resid = resid, a.ldr = ldr, a.y = y, a.ldy = ldy;
  a.rows = rows, a.cg = cg, a.shift = dil * (dir < 0 ? -1 : 1);
  a.relu = relu, a.accumulate = accumulate;
  a.vec = cg % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(wp);
  const int nj = cg > 64 ? 2 : 1;
  a.ntn = cdiv(cg, 64 * nj);
  const dim3 grid(cdiv(rows, GBM), g * a.ntn);
  FX_REQUIRE(grid.y <= 65535u, "grouped conv: too many groups x column tiles");
  if (nj == 2)
    fx_launch(gconv_kernel<2>, grid, dim3(256), 0, s, a);
  else
    fx_launch(gconv_kernel<1>, grid, dim3(256), 0, s, a);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

long long gconv_dw_ws_floats(int rows, int F, int ngroup) {
  const int g = std::max(ngroup, 1);
  if (F < 1 || F % g != 0) return 0;
  int nsplit, rps;
  dw_split(rows, F, g, nsplit, rps);
  return al64((long long)nsplit * 3 * F * (F / g)) + al64((long long)nsplit * F);
}

int launch_gconv_dw(const float* dz, long long lddz, const float* x, long long ldx, int rows, int T, int nvid,
                    const int* seq_off, int F, int ngroup, int dil, float* dw, float* db, float* ws, hipStream_t s) {
  FX_TRY(gconv_check(F, ngroup, "grouped conv dW"));
  FX_REQUIRE(dz && x && ws && rows >= 0 && dil >= 1, "grouped conv dW: bad arguments");
  if (rows == 0 || (!dw && !db)) return FX_OK;
  GDwArgs a{};
  FX_TRY(fill_vidmap(a.vm, rows, T, nvid, seq_off));
  const int g = std::max(ngroup, 1), cg = F / g;
  int nsplit, rps;
  dw_split(rows, F, g, nsplit, rps);
  a.dz = dz, a.lddz = lddz, a.x = x, a.ldx = ldx;
  a.part = ws;
  a.dbpart = db ? ws + al64((long long)nsplit * 3 * F * cg) : nullptr;
  a.rows = rows, a.cg = cg, a.F = F, a.ntc = cdiv(cg, 64), a.dil = dil, a.rows_per_split = rps;
  a.vec = cg % 4 == 0 && ldx % 4 == 0 && lddz % 4 == 0 && aligned16(x) && aligned16(dz);
  const long long gx = (long long)g * a.ntc * a.ntc;
  FX_REQUIRE(gx <= 0x7fffffffLL, "grouped conv dW: too many tiles");
  fx_launch(gconv_dw_kernel, dim3((unsigned)gx, nsplit), dim3(256), 0, s, a);
  FX_CHECK_HIP(hipGetLastError());
  fx_launch(gconv_dw_reduce_kernel, dim3(ew_grid(3LL * F * cg + F)), dim3(256), 0, s, (const float*)a.part,
            (const float*)a.dbpart, nsplit, F, cg, dw, db);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx
