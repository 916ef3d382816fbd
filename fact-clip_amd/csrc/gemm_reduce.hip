// The GEMM's small reductions: the separate split-K reduce launch and the bias-gradient column sums.
#include <algorithm>

#include "gemm_plan.h"

namespace fx {
namespace {

// Separate split-K reduce: a thread sums 4 consecutive elements (float4 over the slabs when M*N % 4 == 0
// and the workspace is 16-B aligned) with up to 8 slab loads in flight, slabs added in order
// (deterministic); the epilogue runs per element.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmDev g, int vec) {
  const long long total = (long long)g.M * g.N;
  const int bidx = blockIdx.y;
  const float* ws = g.ws + (long long)bidx * g.split * total;
  const long long n4 = (total + 3) >> 2;
  for (long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (long long)gridDim.x * blockDim.x) {
    const long long i = i4 * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      for (int k0 = 0; k0 < g.split; k0 += 8) {
        float4 x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          x[j] = *reinterpret_cast<const float4*>(ws + (long long)min(k0 + j, g.split - 1) * total + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (k0 + j < g.split) {
            s[0] += x[j].x;
            s[1] += x[j].y;
            s[2] += x[j].z;
            s[3] += x[j].w;
          }
        }
      }
    } else {
      for (int e = 0; e < 4; ++e)
        if (i + e < total)
          for (int k = 0; k < g.split; ++k) s[e] += ws[(long long)k * total + i + e];
    }
    int m = (int)(i / g.N), n = (int)(i - (long long)m * g.N);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i + e < total) epilogue_store(g, bidx, m, n, s[e]);
      if (++n == g.N) {
        n = 0;
        ++m;
      }
    }
  }
}

// bias-gradient column sums, two deterministic stages (used only where no dW GEMM carries them)
constexpr int CS_ROWS = 128;
// batch z: x + z * x_bs, partials at ws + z * nblk * N, out + z * out_bs
__global__ __launch_bounds__(256) void colsum_stage1(const float* x, long long ld, long long x_bs, int M, int N,
                                                     float* ws) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;
  const int r0 = blockIdx.y * CS_ROWS;
  x += (long long)blockIdx.z * x_bs;
  ws += (long long)blockIdx.z * gridDim.y * N;
  float s = 0.f;
  if (n < N)
    for (int r = r0 + rg; r < min(M, r0 + CS_ROWS); r += 4) s += x[(long long)r * ld + n];
  __shared__ float red[4][64];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && n < N) ws[(long long)blockIdx.y * N + n] = red[0][threadIdx.x] + red[1][threadIdx.x] +
                                                            red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void colsum_stage2(const float* ws, int nblk, int N, float* out, long long out_bs,
                                                     int acc) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  ws += (long long)blockIdx.y * nblk * N;
  out += (long long)blockIdx.y * out_bs;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += ws[(long long)b * N + n];
  out[n] = acc ? out[n] + s : s;
}

}  // namespace

int launch_reduce(const GemmPlan& P, hipStream_t s) {
  if (P.g.split > 1 && !P.g.tile_cnt) {
    const long long total = (long long)P.g.M * P.g.N;
    const int vec = (total % 4) == 0 && ((uintptr_t)P.g.ws & 15) == 0;
    int blocks = (int)std::min<long long>(cdiv(cdiv(total, 4), 256), 2048);
    fx_launch(splitk_reduce_kernel, dim3(blocks, P.batch), dim3(256), 0, s, P.g, vec);
    FX_CHECK_HIP(hipGetLastError());
  }
  return FX_OK;
}

int launch_colsum_batched(const float* x, long long ld, long long x_bs, int M, int N, int nb, float* out,
                          long long out_bs, int accumulate, float* ws, hipStream_t s) {
  if (N == 0 || nb == 0) return FX_OK;
  if (M == 0) {
    if (!accumulate)
      for (int b = 0; b < nb; ++b) FX_CHECK_HIP(hipMemsetAsync(out + (long long)b * out_bs, 0, sizeof(float) * N, s));
    return FX_OK;
  }
  const int nblk = cdiv(M, CS_ROWS);
  fx_launch(colsum_stage1, dim3(cdiv(N, 64), nblk, nb), dim3(256), 0, s, x, ld, x_bs, M, N, ws);
  fx_launch(colsum_stage2, dim3(cdiv(N, 256), nb), dim3(256), 0, s, ws, nblk, N, out, out_bs, accumulate);
  FX_CHECK_HIP(hipGetLastError());
  return FX_OK;
}

int launch_colsum(const float* x, long long ld, int M, int N, float* out, int accumulate, float* ws,
                  hipStream_t s) {
  return launch_colsum_batched(x, ld, 0, M, N, 1, out, 0, accumulate, ws, s);
}

long long colsum_workspace_floats(int M, int N) { return (long long)cdiv(M, CS_ROWS) * N; }

}  // namespace fx

