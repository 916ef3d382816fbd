// X2Y attention core for a SHORT key side (X2Y_map.forward, basic.py:349-389, with X = the action
// tokens: the a2f map of UpdateBlock / UpdateBlockTDU, blocks.py:343-367 and 449-485):
//
//   logit = scale * yq . xk^T      (ny x nx, one video: nx <= 64 keys, ny up to T query rows)
//   attn  = softmax_x(logit)
//   feat  = attn . xv              (ny x Hd)
//
// as ONE launch over every video, instead of a grouped logit GEMM, a softmax launch per video and a
// grouped feat GEMM.  A workgroup (8 waves) owns 32 query rows of one video:
//   1. logits: the 32 x nx tile (<= 2 key blocks of 32) on v_mfma_f32_32x32x2_f32, the Hd-deep sum
//      split over the 8 waves (Hd / 8 each, tile_qk), the 8 partial tiles summed through LDS in wave
//      order (deterministic);
//   2. the row softmax over the nx keys in LDS; logit and attn written (the losses read both);
//   3. feat = attn . xv: 16 column tiles of 32 over Hd = 512, two per wave, K = nx from the LDS
//      probabilities (A) and xv columns (B, 32 lanes read 32 consecutive floats of one key row).
// Algorithmic bytes per 32-row workgroup: yq rows 32 Hd + feat rows 32 Hd (+ logit / attn 2 x 32 nx)
// floats; xk / xv (2 nx Hd floats per video) are L2-resident and shared by every workgroup of the video.
//
// The same core for 65 .. XWMAXK keys per video is the wide variant (calls of <= 64 keys keep the narrow
// kernel).  A workgroup still owns 32 query rows and ALL keys of its video (the softmax runs over the keys):
//   1. loops over PAIRS of 32-key blocks, each pair as above, into the LDS tile P[32][ls], ls = 32 x (key
//      blocks of the call's widest video) + 1;
//   2. loops over the nx keys instead of XMAXK / 16 fixed steps;
//   3. as above (K = nx).
// Its red (64 KB) + P (41 KB at 320 keys) is dynamic LDS above the 64 KB default.
#include "x2y_dev.h"

namespace fx {
namespace {
using namespace x2y_dev;

constexpr int LS = XMAXK + 1;     // LDS row stride of the narrow logit / probability tile
constexpr int XWMAXK = 320;       // keys per video, wide variant
constexpr int XRED = 8 * 2 * 16 * 64;

struct A2fArgs {
  const float* q;       // query-side rows, (Ny, Hd) ld ldq: forward yq, backward dfeat
  long long ldq;
  const float* kmat;    // (Nx, Hd) phase-1 keys: forward xk, backward xv
  const float* vmat;    // (Nx, Hd) phase-3 values: forward xv, backward xk
  const float* attn_in; // backward: the forward's attn (per video (ny_v, nx_v) at aoff[v])
  const float* add_p;   // backward: dattn, added to dP (nullable)
  const float* add_l;   // backward: the direct dlogit, added to the softmax backward (nullable)
  float* out_l;         // forward: logit; backward: dlogit
  float* out_p;         // forward: attn
  float* out_rows;      // (Ny, Hd): forward feat, backward dyq
  int Hd, nvid;
  float scale1, scale3; // forward: logit scale, 1; backward: 1, the logit scale (dyq = scale dlogit . xk)
  X2yVideos vid;        // first[]: first workgroup of each video
};

// f(col) for this thread's columns c0, c0 + 16, ... < nx of a row (16 threads per row)
template <bool WIDE, class F>
__device__ __forceinline__ void a2f_row_cols(int c0, int nx, F&& f) {
  if constexpr (WIDE) {
    for (int col = c0; col < nx; col += 16) f(col);
  } else {
#pragma unroll
    for (int j = 0; j < XMAXK / 16; ++j) {
      const int col = c0 + 16 * j;
      if (col < nx) f(col);
    }
  }
}

// MODE 0: forward (logit, attn, feat); MODE 1: input-gradient side of the backward
//   dP = dfeat . xv^T (+ dattn);  dlogit = attn (dP - sum_x attn dP) (+ direct dlogit);  dyq = scale dlogit . xk
// (the weight-side products dxv = attn^T dfeat and dxk = scale dlogit^T yq reduce over the query rows:
// x2y_a2f_dw_kernel below).
// red: [8][2][16][64] per-wave partial tiles; P: [XR][ls] phase-1 tile, then probabilities / dlogit; rs0 / rs1:
// [XR] forward: row max, row sum; backward: -, row sum of attn dP.  !WIDE: ls = LS and every trip count of
// phases 1 and 2 is a compile-time constant
template <int MODE, bool WIDE>
__device__ __forceinline__ void a2f_body(const A2fArgs& a, float* red, float* P, int ls, float* rs0, float* rs1) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  X2yVideo vd{};
  x2y_block_video(a.vid, a.nvid, blockIdx.x, vd);
  const int y0 = vd.y0, ny = vd.ny, x0 = vd.x0, nx = vd.nx;
  const long long ao = vd.ao;
  const int r0 = ((int)blockIdx.x - vd.first) * XR;     // first query row (video-local)
  const int Hd = a.Hd;
  const int nkb = WIDE ? (nx + 31) >> 5 : (nx > 32 ? 2 : 1);   // 32-key blocks of this video (32 nkb < ls)
  const int rows = min(XR, ny - r0);

  // ---- 1. T = q . kmat^T over Hd, a pair of key blocks at a time (!WIDE: the one pair): wave w sums
  //         k in [w Hd/8, (w+1) Hd/8) ----
  {
    const int kw = Hd >> 3;
    const float* pa = a.q + (long long)(y0 + min(r0 + li, ny - 1)) * a.ldq;
    for (int kp = 0; kp < (WIDE ? nkb : 1); kp += 2) {
      f32x16 acc[2];
      const float* pb[2];
      bool bok[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
        const int key = (kp + c) * 32 + li;
        bok[c] = key < nx;
        pb[c] = a.kmat + (long long)(x0 + min(key, nx - 1)) * Hd;
      }
      tile_qk<2>(pa, li < rows, pb, bok, nkb - kp, w * kw, (w + 1) * kw, lh, acc);
#pragma unroll
      for (int c = 0; c < 2; ++c) red_store(red + (w * 2 + c) * 1024, lane, acc[c]);
      __syncthreads();
      wave_sum(red, 2048, WIDE ? min(2, nkb - kp) * 1024 : 2048, 8, tid, [&](int c, int row, int col, float sum) {
        col += (kp + c) * 32;
        float t = a.scale1 * sum;
        if (MODE == 1 && a.add_p && row < rows && col < nx) t += a.add_p[ao + (long long)(r0 + row) * nx + col];
        P[row * ls + col] = t;
      });
      __syncthreads();   // (red is rewritten by the next pair)
    }
  }

  // ---- 2. per row over the nx keys: 16 threads per row (row tid >> 4, columns (tid & 15) + 16 j) ----
  {
    const int row = tid >> 4, c0 = tid & 15;
    if (MODE == 0) {
      float m = -3.0e38f;
      a2f_row_cols<WIDE>(c0, nx, [&](int col) { m = fmaxf(m, P[row * ls + col]); });
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
      float sum = 0.f;
      a2f_row_cols<WIDE>(c0, nx, [&](int col) { sum += __expf(P[row * ls + col] - m); });
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 16);
      if (c0 == 0) {
        rs0[row] = m;
        rs1[row] = sum;
      }
    } else {
      float sum = 0.f;
      a2f_row_cols<WIDE>(c0, row < rows ? nx : 0, [&](int col) {
        sum += a.attn_in[ao + (long long)(r0 + row) * nx + col] * P[row * ls + col];
      });
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 16);
      if (c0 == 0) rs1[row] = sum;
    }
  }
  __syncthreads();
  const int ncol = WIDE ? nkb << 5 : XMAXK;
  for (int e = tid; e < XR * ncol; e += XT) {
    const int row = e / ncol, col = e - row * ncol;
    float p = 0.f;
    if (col < nx && row < rows) {
      const long long o = ao + (long long)(r0 + row) * nx + col;
      const float t = P[row * ls + col];
      if (MODE == 0) {
        p = __expf(t - rs0[row]) / rs1[row];
        a.out_l[o] = t;
        a.out_p[o] = p;
      } else {
        p = a.attn_in[o] * (t - rs1[row]);
        if (a.add_l) p += a.add_l[o];
        a.out_l[o] = p;
      }
    }
    P[row * ls + col] = p;   // (each element is read and rewritten by the same thread)
  }
  __syncthreads();

  // ---- 3. out rows = scale3 P . vmat: column tiles n0 = 32 (2 w + t), t = 0, 1 ----
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int n0 = 32 * (2 * w + t);
    if (n0 >= Hd) continue;
    f32x16 f;
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = 0.f;
    for (int k0 = 0; k0 < nx; k0 += 32) {
      float bv[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int key = k0 + 16 * lh + s;
        const float x = a.vmat[(long long)(x0 + min(key, nx - 1)) * Hd + n0 + li];
        bv[s] = key < nx ? x : 0.f;
      }
#pragma unroll
      for (int s = 0; s < 16; ++s)
        f = __builtin_amdgcn_mfma_f32_32x32x2f32(P[li * ls + k0 + 16 * lh + s], bv[s], f, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row < rows) a.out_rows[(long long)(y0 + r0 + row) * Hd + n0 + li] = a.scale3 * f[r];
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(XT) void x2y_a2f_kernel(A2fArgs a) {
  __shared__ float red[XRED];
  __shared__ float P[XR * LS];
  __shared__ float rs0[XR], rs1[XR];
  a2f_body<MODE, false>(a, red, P, LS, rs0, rs1);
}

template <int MODE>
__global__ __launch_bounds__(XT) void x2y_a2f_wide_kernel(A2fArgs a, int ls) {
  extern __shared__ float xw_lds[];
  float* P = xw_lds + XRED;
  a2f_body<MODE, true>(a, xw_lds, P, ls, P + XR * ls, P + XR * ls + XR);
}

int launch_a2f(A2fArgs& a, int mode, const int* yoff, const int* xoff, const long long* aoff, hipStream_t s) {
  // an empty key side leaves no workgroup: softmax over nothing has no rows to write
  const int wg = x2y_fill_videos(a.vid, a.nvid, yoff, xoff, aoff,
                                 [](int ny, int nx) { return nx > 0 ? (ny + XR - 1) / XR : 0; });
  const int nxmax = x2y_max_rows(a.nvid, xoff);
  if (wg == 0) return FX_OK;
  if (nxmax > XMAXK) {
    // the wide variant: P rows of the widest video's key blocks, dynamic LDS above the 64 KB default
    constexpr int kMaxLds = (XRED + XR * (XWMAXK + 1) + 2 * XR) * (int)sizeof(float);
    static const bool attr = [] {
      return hipFuncSetAttribute((const void*)x2y_a2f_wide_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kMaxLds) == hipSuccess &&
             hipFuncSetAttribute((const void*)x2y_a2f_wide_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kMaxLds) == hipSuccess;
    }();
    FX_REQUIRE(attr, "x2y a2f core: cannot raise the LDS limit");
    const int ls = ((nxmax + 31) / 32) * 32 + 1;
    const std::uint32_t shm = (std::uint32_t)((XRED + XR * ls + 2 * XR) * sizeof(float));
    if (mode == 0)
      fx_launch(x2y_a2f_wide_kernel<0>, dim3(wg), dim3(XT), shm, s, a, ls);
    else
      fx_launch(x2y_a2f_wide_kernel<1>, dim3(wg), dim3(XT), shm, s, a, ls);
  } else if (mode == 0) {
    fx_launch(x2y_a2f_kernel<0>, dim3(wg), dim3(XT), 0, s, a);
  } else {
    fx_launch(x2y_a2f_kernel<1>, dim3(wg), dim3(XT), 0, s, a);
  }
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace

static_assert(XWMAXK == FX_X2Y_MAXTOK && XWMAXK % 32 == 0, "wide a2f core: key blocks of 32 up to FX_X2Y_MAXTOK");

bool x2y_a2f_fusable(int nvid, const int* xoff, int Hd) { return a2f_fits(nvid, xoff, Hd, XMAXK); }

int launch_x2y_a2f_fwd(const float* yq, const float* xk, const float* xv, int Hd, float scale, int nvid,
                       const int* yoff, const int* xoff, const long long* aoff, float* logit, float* attn,
                       float* feat, hipStream_t s) {
  FX_REQUIRE(a2f_fits(nvid, xoff, Hd, XWMAXK), "x2y a2f core: <= 320 keys per video, Hd % 256 == 0, <= 16 videos");
  A2fArgs a{};
  a.q = yq;
  a.ldq = Hd;
  a.kmat = xk;
  a.vmat = xv;
  a.out_l = logit;
  a.out_p = attn;
  a.out_rows = feat;
  a.Hd = Hd;
  a.nvid = nvid;
  a.scale1 = scale;
  a.scale3 = 1.f;
  return launch_a2f(a, 0, yoff, xoff, aoff, s);
}

int launch_x2y_a2f_bwd(const float* dfeat, long long ldf, const float* xv, const float* xk, const float* attn,
                       const float* dattn, const float* dlogit_in, int Hd, float scale, int nvid, const int* yoff,
                       const int* xoff, const long long* aoff, float* dlogit, float* dyq, hipStream_t s) {
  FX_REQUIRE(a2f_fits(nvid, xoff, Hd, XWMAXK), "x2y a2f core: <= 320 keys per video, Hd % 256 == 0, <= 16 videos");
  FX_REQUIRE(ldf % 4 == 0 && (reinterpret_cast<uintptr_t>(dfeat) & 15) == 0, "x2y a2f bwd: dfeat rows must be 16-B aligned");
  A2fArgs a{};
  a.q = dfeat;
  a.ldq = ldf;
  a.kmat = xv;
  a.vmat = xk;
  a.attn_in = attn;
  a.add_p = dattn;
  a.add_l = dlogit_in;
  a.out_l = dlogit;
  a.out_rows = dyq;
  a.Hd = Hd;
  a.nvid = nvid;
  a.scale1 = 1.f;
  a.scale3 = scale;
  return launch_a2f(a, 1, yoff, xoff, aoff, s);
}

// ---------------------------------------------------------------- a2f weight-side products
// dxv = attn^T dfeat and dxk = scale dlogit^T yq of every video (the products of the a2f backward that
// reduce over the query rows) in ONE launch, instead of grouped split-K GEMMs + their reduce launches:
// grid (row chunk, 32-column block of Hd, video x {dxv, dxk}); a workgroup's 4 waves each take a quarter
// of the chunk's rows (sub-chunks of 32: the P values of a row as the A operand with the key as the row
// index -- lane li reads P[r][li], 32 lanes one 128-B row slice --, the B rows likewise), summed through
// LDS in wave order; the chunks of a (video, matrix, column block) are summed in chunk order by the last
// workgroup to finish one (write-through hand-off: partials stored sc1 and acknowledged before the
// arrival, read back sc1 by the last arriver, which re-arms the counter) -- deterministic.
// WIDE (65 .. 320 keys per video): the 64-key blocks of the output are independent -- grid y becomes
// (key block, column block), and the counter groups and partial slabs grow by the key blocks.
namespace {
constexpr int DWT = 256;          // threads
constexpr int DW_MAXC = 8;        // row chunks per video
struct A2fDwArgs {
  const float* attn;              // per video (ny x nx) at aoff[v]
  const float* dl;                // dlogit, same layout
  const float* dfeat;             // (Ny, Hd) rows, ld ldf
  long long ldf;
  const float* yq;                // (Ny, Hd) rows, ld Hd
  float* dxv;                     // (Nx, Hd) rows
  float* dxk;
  float scale;
  int Hd, nvid, nchunk, crows;    // chunks per video (grid x), rows per chunk (a multiple of 128)
  int nkb;                        // 64-key blocks of the widest video (WIDE; else 1)
  float* ws;                      // partials [vid][mat][key block][col block][chunk][64 x][32 d]
  unsigned* cnt;                  // arrival counters [vid][mat][key block][col block]
  X2yVideos vid;                  // (first[] unused: the video is a grid dimension)
};

template <bool WIDE>
__global__ __launch_bounds__(DWT) void x2y_a2f_dw_kernel(A2fDwArgs a) {
  __shared__ float red[4][2][16][64];
  __shared__ int last;
  const int ncb = WIDE ? a.Hd >> 5 : (int)gridDim.y;
  const int kb = WIDE ? (int)blockIdx.y / ncb : 0;     // 64-key block of the output
  const int c = blockIdx.x, cb = WIDE ? (int)blockIdx.y - kb * ncb : (int)blockIdx.y, vid = blockIdx.z >> 1,
            mat = blockIdx.z & 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  X2yVideo vd{};
  x2y_video(a.vid, vid, vd);
  const int y0 = vd.y0, ny = vd.ny, x0 = vd.x0, nxv = vd.nx;
  const long long ao = vd.ao;
  const int xb = WIDE ? 64 * kb : 0;                  // first key of the block (video-local)
  const int nx = WIDE ? min(64, nxv - xb) : nxv;      // keys of the block
  if (nx <= 0 || ny <= 0) return;                     // (uniform: the whole workgroup)
  const int nch = (ny + a.crows - 1) / a.crows;       // this video's chunks
  if (c >= nch) return;
  const float* P = (mat == 0 ? a.attn : a.dl) + ao + xb;   // (ny x nxv), the block's columns
  const float* B = mat == 0 ? a.dfeat : a.yq;
  const long long ldb = mat == 0 ? a.ldf : a.Hd;
  const int d0 = cb * 32;
  const int nxt = nx > 32 ? 2 : 1;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  // this wave's rows: [c crows + w crows/4, + crows/4) in sub-chunks of 32 (lane half lh: rows 16 lh ..
  // + 15): the P values of a row as the A operand with the key as the row index (lane li reads P[r][li],
  // 32 lanes one 128-B row slice), the B rows likewise.  (Staging the chunk through LDS first, and a
  // register double buffer over the sub-chunks, both measured slower.)
  const int wr0 = c * a.crows + w * (a.crows >> 2), wr1 = min(ny, wr0 + (a.crows >> 2));
  for (int r0 = wr0; r0 < wr1; r0 += 32) {
    float pv[2][16], bv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int r = r0 + 16 * lh + s, rc = min(r, ny - 1);
      bv[s] = B[(long long)(y0 + rc) * ldb + d0 + li];
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < nxt) pv[t][s] = P[(long long)rc * nxv + min(32 * t + li, nx - 1)];
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const bool rok = r0 + 16 * lh + s < wr1;
      const float b = rok ? bv[s] : 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < nxt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(32 * t + li < nx ? pv[t][s] : 0.f, b, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[w][t][r][lane] = acc[t][r];
  __syncthreads();
  // the workgroup's tile (64 x, 32 d) summed over the waves in order; thread -> 8 elements (t, r, lane)
  const float mul = mat == 0 ? 1.f : a.scale;
  float* out = mat == 0 ? a.dxv : a.dxk;
  const long long grp = WIDE ? (((long long)vid * 2 + mat) * a.nkb + kb) * ncb + cb
                             : ((long long)vid * 2 + mat) * gridDim.y + cb;
  float* part = a.ws + (grp * a.nchunk + c) * 2048;
  const bool direct = nch == 1 || a.cnt == nullptr;
  float v8[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = tid + i * DWT, t = e >> 10, r = (e >> 6) & 15, l = e & 63;
    v8[i] = (red[0][t][r][l] + red[1][t][r][l]) + (red[2][t][r][l] + red[3][t][r][l]);
    const int x = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), d = d0 + (l & 31);
    if (direct) {
      if (x < nx && t < nxt) out[(long long)(x0 + xb + x) * a.Hd + d] = v8[i] * mul;
    } else {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v8[i]), rsrc(part), e * 4, 0, 16);
    }
  }
  if (direct) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's partial stores acknowledged
  __syncthreads();
  if (tid == 0) {
    unsigned* cp = a.cnt + grp;
    const unsigned prev = __hip_atomic_fetch_add(cp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == (unsigned)nch - 1;
    if (last) __hip_atomic_store(cp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  const float* pbase = a.ws + grp * a.nchunk * 2048;
  float x8[DW_MAXC][8];
#pragma unroll
  for (int q = 0; q < DW_MAXC; ++q)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      x8[q][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
          rsrc(pbase), ((long long)min(q, nch - 1) * 2048 + tid + i * DWT) * 4, 0, 16));
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = tid + i * DWT, t = e >> 10, r = (e >> 6) & 15, l = e & 63;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < DW_MAXC; ++q)
      if (q < nch) sum += x8[q][i];
    const int x = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), d = d0 + (l & 31);
    if (x < nx && t < nxt) out[(long long)(x0 + xb + x) * a.Hd + d] = sum * mul;
  }
}

// row chunks per video aimed at for `groups` counter groups: about one workgroup per CU
int dw_chunks(long long groups) {
  return (int)std::max<long long>(1, std::min<long long>(DW_MAXC, (256 + groups - 1) / groups));
}
int dw_key_blocks(int nvid, const int* xoff) { return std::max(1, (x2y_max_rows(nvid, xoff) + 63) / 64); }
}  // namespace

bool x2y_a2f_dw_ok(int nvid, const int* yoff) {
  (void)yoff;   // (any row count: the chunks grow with the video)
  return nvid >= 1 && nvid <= FX_X2Y_MAXV;
}
long long x2y_a2f_dw_ws_floats(int nvid, int Hd, const int* xoff) {
  const int nkb = dw_key_blocks(nvid, xoff);
  const long long groups = (long long)nvid * 2 * (Hd / 32);
  // (videos past the wide core's keys never reach the kernel: sized as one key block)
  if (nkb == 1 || nkb > FX_X2Y_MAXTOK / 64) return groups * DW_MAXC * 2048;
  return groups * nkb * dw_chunks(groups * nkb) * 2048;
}

int launch_x2y_a2f_dw(const float* attn, const float* dl, const float* dfeat, long long ldf, const float* yq, int Hd,
                      float scale, int nvid, const int* yoff, const int* xoff, const long long* aoff, float* dxv,
                      float* dxk, float* ws, hipStream_t s) {
  FX_REQUIRE(nvid >= 1 && nvid <= FX_X2Y_MAXV && Hd % 32 == 0, "x2y a2f dW: <= 16 videos, Hd % 32 == 0");
  FX_REQUIRE(x2y_max_rows(nvid, xoff) <= FX_X2Y_MAXTOK, "x2y a2f dW: <= 320 keys per video");
  A2fDwArgs a{};
  a.attn = attn;
  a.dl = dl;
  a.dfeat = dfeat;
  a.ldf = ldf;
  a.yq = yq;
  a.dxv = dxv;
  a.dxk = dxk;
  a.scale = scale;
  a.Hd = Hd;
  a.nvid = nvid;
  x2y_fill_videos(a.vid, nvid, yoff, xoff, aoff, [](int, int) { return 0; });
  const int nymax = x2y_max_rows(nvid, yoff);
  if (nymax == 0) return FX_OK;
  // about one workgroup per CU: chunks of a multiple of 128 rows (32 per wave), at most DW_MAXC per video
  const int ncb = Hd / 32;
  const int nkb = dw_key_blocks(nvid, xoff);
  const long long groups = (long long)nvid * 2 * ncb * nkb;
  // (more groups than arrival counters: one chunk, which needs neither counters nor partials)
  int nchunk = groups <= kArrivalCounters ? dw_chunks(groups) : 1;
  int crows = (nymax + nchunk - 1) / nchunk;
  crows = (crows + 127) / 128 * 128;
  nchunk = (nymax + crows - 1) / crows;
  a.nchunk = nchunk;
  a.crows = crows;
  a.nkb = nkb;
  a.ws = ws;
  a.cnt = (nchunk > 1 && groups <= kArrivalCounters) ? arrival_counters(s) : nullptr;
  FX_REQUIRE(nchunk == 1 || (a.cnt && ws), "x2y a2f dW: workspace / counters required");
  if (nkb == 1)
    fx_launch(x2y_a2f_dw_kernel<false>, dim3(nchunk, ncb, 2 * nvid), dim3(DWT), 0, s, a);
  else
    fx_launch(x2y_a2f_dw_kernel<true>, dim3(nchunk, ncb * nkb, 2 * nvid), dim3(DWT), 0, s, a);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // namespace fx
