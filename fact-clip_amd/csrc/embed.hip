// Token embedding of a transcript-conditioned model (blocks.py:75-79): the action tokens are the embedded
// transcript entries of the stacked videos plus the positional rows of their places in each transcript.
//   forward   out[r, :] = W[ids[r], :] + pe[pos[r], :]          (pe nullable)
//   backward  dW[c, :] (+)= sum of dout[r, :] over the rows r with ids[r] == c, in increasing r
// The backward gathers: the transcript is known on the host, which passes the class -> rows grouping as a
// CSR pair (coff[C + 1], clist[R]); one thread owns one (class, column) element and adds its rows in list
// order, so there is no float atomic and the result is bitwise repeatable.
#include <algorithm>

#include "fx_common.h"
#include "ops.h"

namespace fx {
namespace {

constexpr int ET = 256;

__global__ __launch_bounds__(ET) void token_embed_fwd_kernel(const float* W, long long ldw, int C, int A,
                                                             const int32_t* ids, const int32_t* pos, int R,
                                                             const float* pe, long long ldpe, int npe, float* out,
                                                             long long ldo) {
  const long long e = (long long)blockIdx.x * ET + threadIdx.x;
  if (e >= (long long)R * A) return;
  const int r = (int)(e / A), a = (int)(e - (long long)r * A);
  const int c = min(max(ids[r], 0), C - 1);          // (range-checked on the host copy; never out of bounds)
  float y = W[(long long)c * ldw + a];
  if (pe) y += pe[(long long)min(max(pos[r], 0), npe - 1) * ldpe + a];
  out[(long long)r * ldo + a] = y;
}

__global__ __launch_bounds__(ET) void token_embed_bwd_kernel(const float* dout, long long ldd, int R, int A,
                                                             const int32_t* coff, const int32_t* clist, float* dW,
                                                             long long lddw, int accumulate) {
  const int c = blockIdx.y;
  const int a = blockIdx.x * ET + threadIdx.x;
  if (a >= A) return;
  const int lo = coff[c], hi = coff[c + 1];
  if (accumulate && hi <= lo) return;
  float s = 0.f;
  for (int i = lo; i < hi; ++i) {
    const int r = min(max(clist[i], 0), R - 1);
    s += dout[(long long)r * ldd + a];
  }
  float* d = dW + (long long)c * lddw + a;
  *d = accumulate ? *d + s : s;
}

}  // namespace
}  // namespace fx

using namespace fx;

extern "C" {

int fx_token_embed_fwd(const float* W, long long ldw, int C, int A, const int32_t* ids_host,
                       const int32_t* pos_host, const int32_t* ids_dev, const int32_t* pos_dev, int R,
                       const float* pe, long long ldpe, int npe, float* out, long long ldo, void* stream) {
  FX_REQUIRE(W && ids_host && ids_dev && out && C > 0 && A > 0 && R >= 0 && ldw >= A && ldo >= A,
             "token_embed: bad arguments");
  FX_REQUIRE(!pe || (pos_host && pos_dev && npe > 0 && ldpe >= A), "token_embed: positions without their table");
  for (int r = 0; r < R; ++r) {
    FX_REQUIRE(ids_host[r] >= 0 && ids_host[r] < C, "token_embed: class id out of range");
    FX_REQUIRE(!pe || (pos_host[r] >= 0 && pos_host[r] < npe), "token_embed: position out of range");
  }
  if (R == 0) return FX_OK;
  fx_launch(token_embed_fwd_kernel, dim3(cdiv((long long)R * A, ET)), dim3(ET), 0, (hipStream_t)stream, W, ldw, C, A,
            ids_dev, pos_dev, R, pe, ldpe, npe, out, ldo);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int fx_token_embed_bwd(const float* dout, long long ldd, int R, int C, int A, const int32_t* coff_host,
                       const int32_t* clist_host, const int32_t* coff_dev, const int32_t* clist_dev, float* dW,
                       long long lddw, int accumulate, void* stream) {
  FX_REQUIRE(dout && coff_host && clist_host && coff_dev && clist_dev && dW && C > 0 && A > 0 && R > 0 && ldd >= A &&
                 lddw >= A,
             "token_embed_bwd: bad arguments");
  FX_REQUIRE(C <= 65535, "token_embed_bwd: more than 65535 classes");
  FX_REQUIRE(coff_host[0] == 0 && coff_host[C] == R, "token_embed_bwd: the class offsets must cover the R rows");
  for (int c = 0; c < C; ++c) {
    FX_REQUIRE(coff_host[c] <= coff_host[c + 1] && coff_host[c + 1] <= R,
               "token_embed_bwd: class offsets must not decrease");
    for (int i = coff_host[c]; i < coff_host[c + 1]; ++i) {
      FX_REQUIRE(clist_host[i] >= 0 && clist_host[i] < R, "token_embed_bwd: row out of range");
      FX_REQUIRE(i == coff_host[c] || clist_host[i] > clist_host[i - 1],
                 "token_embed_bwd: a class's rows must increase");
    }
  }
  fx_launch(token_embed_bwd_kernel, dim3(cdiv(A, ET), C), dim3(ET), 0, (hipStream_t)stream, dout, ldd, R, A, coff_dev,
            clist_dev, dW, lddw, accumulate);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

}  // extern "C"
