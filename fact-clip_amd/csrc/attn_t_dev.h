// Pieces shared by the two kernel families of the attention of a few queries over T frames
// (attn_t_lds.hip: operands staged in LDS; attn_t_rr.hip: operands in MFMA registers, head dim 32) and by
// the host code that plans and issues their launches (attention.cpp): the argument block, the layout of
// the partial workspace, the chunk a workgroup owns, the dropout mask, and the families' launchers.
#pragma once
#include "fx_common.h"
#include "wave_dev.h"

namespace fx {
namespace attn_t_dev {

constexpr int AT = 256;        // threads per workgroup (4 waves)
constexpr int MAXV = 32;       // videos per launch (per-video key row offsets live in the kernel arguments)
constexpr int QB = 64;         // queries per launch (query blocks of more tokens run as successive launches)
constexpr int NVK = 8;         // LDS-staged kernels: float4 per thread of a staged K / V chunk
constexpr int FOLD_MAX = 16;   // chunks per video merged inside the launch (more: tattn_merge_kernel)

struct TAttnArgs {
  const float* q; long long ldq;
  const float* k; long long ldk;
  const float* v; long long ldv;
  const float* o; long long ldo;        // bwd: forward output
  const float* dout; long long lddo;    // bwd
  float* out; long long ld_out;         // fwd: o;  bwd: dq
  float* dk; long long lddk;            // bwd
  float* dv; long long lddv;            // bwd
  float* lse;                           // (nvid, h, qs): fwd writes, bwd reads
  float* ws;                            // partials (TAttnWs)
  int Qv, hd, nh, Qp, Hp, Tc, nsplit;   // Qv: queries of this block (longest video); nsplit: max chunks over the videos
  int qs, q0;                           // longest video's query rows (lse stride), first query of the block
  int acc_kv;                           // bwd: dK / dV += (later query blocks of the same keys)
  float scale;
  int vec;                              // 16-B loads of every q / k / v / o / dout row slice
  float drop_p;                         // attention-probability dropout (training), counter-based mask
  unsigned drop_thr;
  unsigned long long drop_seed;
  long long ktot;                       // key rows over all videos (mask index stride)
  unsigned* cnt;                        // register-resident kernels: arrival counters per (video, head) for the
                                        // in-launch merge (null: partials for tattn_merge_kernel)
  int koff[MAXV + 1];                   // key / value rows of video v: [koff[v], koff[v+1])
  int qoff[MAXV + 1];                   // query rows of video v: [qoff[v], qoff[v+1])
};

// The partial workspace of one launch of nsplit > 1 chunks: np = nvid nh nsplit partials, (video, head,
// chunk) at pid; the np (Qp x Hp) tiles, then the np rows of m, then the np rows of l (forward only).
// Every kernel addresses it through this, and the host sizes it with floats().
struct TAttnWs {
  long long np;
  int Qp, Hp;
  __host__ __device__ TAttnWs(int nvid, int nh, int nsplit, int Qp_, int Hp_)
      : np((long long)nvid * nh * nsplit), Qp(Qp_), Hp(Hp_) {}
  __host__ __device__ static long long pid(int vid, int nh, int h, int nsplit, int c) {
    return ((long long)vid * nh + h) * nsplit + c;
  }
  __host__ __device__ long long tile(long long p) const { return p * Qp * Hp; }   // first float of tile p
  __host__ __device__ long long at(long long p, int row, int col) const { return (p * Qp + row) * Hp + col; }
  __host__ __device__ long long m() const { return np * Qp * Hp; }                // row r of partial p: [p * Qp + r]
  __host__ __device__ long long l() const { return m() + np * Qp; }
  __host__ __device__ long long floats() const { return l() + np * Qp; }
};

// live queries of video vid in the launch's query block [q0, q0 + Qv): 0 when the video is shorter than q0
__device__ __forceinline__ int live_queries(const TAttnArgs& a, int vid) {
  return max(0, min(a.Qv, a.qoff[vid + 1] - a.qoff[vid] - a.q0));
}

// The chunk of workgroup (chunk c, video vid): nk keys from key row krow (t0 of the video's Tv), the Qn
// live queries of the block from query row qrow.  nk <= 0: the video has no such chunk (a shorter video of
// a ragged batch has fewer) and the workgroup leaves.
struct TAttnChunk {
  int Tv, t0, nk, Qn;
  long long qrow, krow;
};
__device__ __forceinline__ TAttnChunk tattn_chunk(const TAttnArgs& a, int c, int vid) {
  TAttnChunk k;
  k.Tv = a.koff[vid + 1] - a.koff[vid];
  k.t0 = c * a.Tc;
  k.nk = min(a.Tc, k.Tv - k.t0);
  k.Qn = live_queries(a, vid);
  k.qrow = (long long)a.qoff[vid] + a.q0;
  k.krow = (long long)a.koff[vid] + k.t0;
  return k;
}

// keep-scale of probability (global query row qg, head h, global key row kg): 1/(1-p) or 0
__device__ __forceinline__ float drop_keep(const TAttnArgs& a, long long qg, int h, long long kg) {
  const unsigned long long idx = ((unsigned long long)qg * a.nh + h) * (unsigned long long)a.ktot + kg;
  return fx_drop_bits(a.drop_seed, idx) >= a.drop_thr ? 1.f / (1.f - a.drop_p) : 0.f;
}

// ---- host: one launch each, the caller checks hipGetLastError.  grid = (chunks, heads, videos); a carries
// the query block (q0, Qv, acc_kv).
// attn_t_lds.hip: tattn_fwd_kernel / tattn_bwd_kernel with `lds` bytes of dynamic LDS
void launch_tattn_lds(const TAttnArgs& a, bool bwd, dim3 grid, size_t lds, hipStream_t s);
// attn_t_lds.hip: tattn_merge_kernel over the partials either family left, one workgroup per (head, video);
// stats: the forward's weights from (m, l) and lse, `lds` bytes for them; else out = mul * sum
void launch_tattn_merge(const TAttnArgs& a, int nvid, bool stats, float mul, size_t lds, hipStream_t s);
// attn_t_rr.hip: tattn_fwd32_kernel<KT> / tattn_bwd32_kernel<KT>, 32 KT keys per wave (Tc = 128 KT)
void launch_tattn_rr(const TAttnArgs& a, bool bwd, int KT, dim3 grid, hipStream_t s);

}  // namespace attn_t_dev
}  // namespace fx
