// GEMM host side: launch_gemm / launch_gemm_group (plan, census line, the family's launcher, reduce),
// the arrival-counter pool, the workspace bound, the descriptor helpers and the per-stream precision.
// The decisions are in gemm_plan.cpp, the kernels in gemm_<family>.hip.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "gemm_plan.h"

namespace fx {

// Split-K arrival counters, one pool per (device, stream): zeroed once at allocation and
// re-armed by the last block of every tile, so launches on one stream reuse them safely.
unsigned* arrival_counters(hipStream_t s) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, unsigned*> pool;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_pair(dev, s);
  auto it = pool.find(key);
  if (it != pool.end()) return it->second;
  unsigned* p = nullptr;
  if (hipMalloc(&p, kArrivalCounters * sizeof(unsigned)) != hipSuccess) return nullptr;
  if (hipMemsetAsync(p, 0, kArrivalCounters * sizeof(unsigned), s) != hipSuccess) {
    (void)hipFree(p);
    return nullptr;
  }
  pool[key] = p;
  return p;
}

thread_local const float* t_ws_lo = nullptr;
thread_local const float* t_ws_hi = nullptr;

WsBound::WsBound(const float* base, long long floats) : prev_lo(t_ws_lo), prev_hi(t_ws_hi) {
  t_ws_lo = base;
  t_ws_hi = base ? base + std::max(floats, 0LL) : nullptr;
}
WsBound::~WsBound() {
  t_ws_lo = prev_lo;
  t_ws_hi = prev_hi;
}

fx_operand op_rows(const float* p, long long ld) {
  fx_operand o{};
  o.ptr = p;
  o.ld = ld;
  o.conv_dir = 1;
  return o;
}

fx_operand op_cols(const float* p, long long ld) {
  fx_operand o = op_rows(p, ld);
  o.trans = 1;
  return o;
}

fx_gemm_desc gemm_desc(int M, int N, int K, fx_operand a, fx_operand b, float* c, long long ldc) {
  fx_gemm_desc d{};
  d.M = M;
  d.N = N;
  d.K = K;
  d.batch = 1;
  d.a = a;
  d.b = b;
  d.c = c;
  d.ldc = ldc;
  d.alpha = 1.f;
  d.split_k = 1;
  return d;
}

long long gemm_workspace_floats(const fx_gemm_desc& d) {
  if (d.split_k <= 1) return 0;
  return (long long)d.batch * d.split_k * d.M * d.N;
}

// GEMM arithmetic precision per caller stream (fx_set_stream_precision): a few (stream, precision)
// pairs behind a mutex; streams never set run FX_PREC_F32.  Per stream, so two callers with different
// precisions on different streams (or threads) do not interfere.
std::mutex g_prec_mu;
std::vector<std::pair<hipStream_t, int>> g_prec;
std::atomic<int> g_prec_any{0};   // fast path: no stream has an explicit setting
std::atomic<int> g_prec_default{FX_PREC_F32};   // streams without one (fx_set_default_precision)

int stream_precision(hipStream_t s) {
  if (!g_prec_any.load(std::memory_order_acquire)) return g_prec_default.load(std::memory_order_relaxed);
  std::lock_guard<std::mutex> lk(g_prec_mu);
  for (const auto& e : g_prec)
    if (e.first == s) return e.second;
  return g_prec_default.load(std::memory_order_relaxed);
}

bool valid_precision(int prec) {
  return prec == FX_PREC_F32 || prec == FX_PREC_BF16 || prec == FX_PREC_F32S || prec == FX_PREC_F32S2;
}

namespace {

// The plan of d on stream s (member of a grouped launch: counters from cnt_base on), checked against the
// entry point's workspace reservation, with the stream's arrival counters attached where the plan wants
// the in-launch reduction; without a pool the separate reduce launch follows.
int plan_on_stream(const fx_gemm_desc& d, hipStream_t s, long long cnt_base, GemmPlan& P) {
  FX_TRY(plan_gemm(d, stream_precision(s), knobs(), cnt_base, P));
  GemmDev& g = P.g;
  const bool direct = P.family == FAM_DIRECT;
  const int cap = d.split_k > 1 ? d.split_k : 1;
  if (g.split > 1 && t_ws_hi && !(g.ws >= t_ws_lo && g.ws + (long long)g.split * d.M * d.N * d.batch <= t_ws_hi))
    std::fprintf(stderr, "factmx: gemm M %d N %d K %d batch %d split %d (cap %d, %s) needs %lld floats at +%lld of a %lld-float reservation\n",
                 d.M, d.N, d.K, d.batch, g.split, cap, direct ? "direct" : "tiled",
                 (long long)g.split * d.M * d.N * d.batch, (long long)(g.ws - t_ws_lo), (long long)(t_ws_hi - t_ws_lo));
  FX_REQUIRE(g.split <= 1 || !t_ws_hi ||
                 (g.ws >= t_ws_lo && g.ws + (long long)g.split * d.M * d.N * d.batch <= t_ws_hi),
             "gemm: split-K slabs would overrun the entry point's workspace reservation");
  if (P.counters) {
    unsigned* pool = arrival_counters(s);
    g.tile_cnt = pool ? pool + P.cnt_base : nullptr;
  }
  return FX_OK;
}

// diagnostic build only (-DFX_GEMM_CENSUS, tools/r06_gemm_census.sh): one line per GEMM kernel launch, in
// launch order
void census(const fx_gemm_desc& d, const GemmPlan& P, hipStream_t s) {
#ifdef FX_GEMM_CENSUS
  std::fprintf(stderr, "GEMM %p %d %d %d %d %d %d %d %d %d %d %d\n", (void*)s, d.M, d.N, d.K, d.batch, P.ak, P.bk,
               P.g.split, P.family == FAM_DIRECT ? 1 : P.family == FAM_TILED ? 0 : 2, P.g.persist, d.a.conv_taps,
               (int)(P.g.split > 1 && !P.g.tile_cnt));
#endif
}

int launch_family(const GemmPlan& P, hipStream_t s) {
  switch (P.family) {
    case FAM_TILED: return launch_tiled(P, s);
    case FAM_WIDE8: return launch_wide8(P, s);
    case FAM_BF16: return launch_bf16(P, s);
    case FAM_SPLIT: return launch_split(P, s);
    case FAM_DIRECT: return launch_direct(P, s);
    default: break;
  }
  set_error("gemm: unknown kernel family");
  return FX_ERR_UNSUPPORTED;
}

}  // namespace

int launch_gemm(const fx_gemm_desc& d, hipStream_t s) {
  FX_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0 && d.batch >= 1, "gemm: bad sizes");
  if (d.M == 0 || d.N == 0) return FX_OK;
  GemmPlan P;
  FX_TRY(plan_on_stream(d, s, 0, P));
  census(d, P, s);
  FX_TRY(launch_family(P, s));
  FX_CHECK_HIP(hipGetLastError());
  return launch_reduce(P, s);
}

// Independent GEMMs (no member reads another's output; disjoint outputs and workspaces) in one
// launch when every member takes the direct kernel; otherwise one launch each, in order.
// FX_GEMM_GROUP=0 disables the grouping (diagnostic A/B).
int launch_gemm_group(const fx_gemm_desc* d, int n, hipStream_t s) {
  const bool on = knobs().gemm_group;
  FX_REQUIRE(n >= 0 && n <= GMAX, "gemm group: 0..4 members");
  int live = 0, nsplit = 0;   // members with M, N > 0; of those, split-K members
  bool all_direct = on;
  GemmPlan P[GMAX];
  long long cnt_base = 0;
  for (int i = 0; i < n && all_direct; ++i) {
    FX_REQUIRE(d[i].M >= 0 && d[i].N >= 0 && d[i].K >= 0 && d[i].batch >= 1, "gemm: bad sizes");
    if (d[i].M == 0 || d[i].N == 0) continue;
    FX_TRY(plan_on_stream(d[i], s, cnt_base, P[i]));
    if (P[i].g.tile_cnt) cnt_base += P[i].counters;
    all_direct = all_direct && P[i].family == FAM_DIRECT;
    nsplit += P[i].g.split > 1 ? 1 : 0;
    ++live;
  }
  // split members given the same workspace get consecutive slab ranges in it (checked against the
  // entry point's reservation); split members on different workspaces are not grouped
  bool ws_ok = true;
  if (all_direct && nsplit > 1) {
    const float* base = nullptr;
    long long off = 0;
    for (int i = 0; i < n && ws_ok; ++i) {
      if (d[i].M == 0 || d[i].N == 0 || P[i].g.split <= 1) continue;
      if (!base) base = d[i].workspace;
      ws_ok = d[i].workspace == base && t_ws_hi != nullptr;
      P[i].g.ws = d[i].workspace + off;
      off += (long long)P[i].g.split * d[i].M * d[i].N * d[i].batch;
      ws_ok = ws_ok && P[i].g.ws >= t_ws_lo && P[i].g.ws + (long long)P[i].g.split * d[i].M * d[i].N * d[i].batch <= t_ws_hi;
    }
  }
  if (!all_direct || live < 2 || !ws_ok) {
    for (int i = 0; i < n; ++i) FX_TRY(launch_gemm(d[i], s));
    return FX_OK;
  }
  // one launch per distinct block size: a member planned with fewer waves per tile would otherwise run
  // with idle waves in every block (measured: a K = 32 member beside a K = 4096 one, 2x slower)
  bool done[GMAX] = {};
  for (int i0 = 0; i0 < n; ++i0) {
    if (done[i0] || d[i0].M == 0 || d[i0].N == 0) continue;
    const unsigned nw = P[i0].block.x;
    GemmGroup G{};
    int m = 0;
    G.start[0] = 0;
    for (int i = i0; i < n; ++i) {
      if (done[i] || d[i].M == 0 || d[i].N == 0 || P[i].block.x != nw) continue;
      done[i] = true;
      G.g[m] = P[i].g;
      G.kinds[m] = gen_kind(P[i].ak) * 8 + P[i].bk;
      G.start[m + 1] = G.start[m] + (int)(P[i].grid.x * P[i].grid.y * P[i].grid.z);
      ++m;
    }
    for (int i = m + 1; i <= GMAX; ++i) G.start[i] = G.start[m];
    G.n = m;
    if (m == 1) {
      census(d[i0], P[i0], s);
      FX_TRY(launch_direct(P[i0], s));
    } else {
      launch_direct_group(G, G.start[m], nw, s);
    }
    FX_CHECK_HIP(hipGetLastError());
  }
  for (int i = 0; i < n; ++i)
    if (d[i].M != 0 && d[i].N != 0) FX_TRY(launch_reduce(P[i], s));
  return FX_OK;
}

}  // namespace fx

extern "C" {

// The plan of desc as launch_gemm would make it on a stream of precision prec (host only)
int fx_gemm_plan(const fx_gemm_desc* desc, int prec, fx_gemm_plan_info* out) {
  FX_REQUIRE(desc && out, "fx_gemm_plan: null argument");
  FX_REQUIRE(fx::valid_precision(prec), "fx_gemm_plan: FX_PREC_F32, FX_PREC_BF16, FX_PREC_F32S or FX_PREC_F32S2");
  *out = fx_gemm_plan_info{};
  const fx_gemm_desc& d = *desc;
  FX_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0 && d.batch >= 1, "gemm: bad sizes");
  if (d.M == 0 || d.N == 0) return FX_OK;
  fx::GemmPlan P;
  FX_TRY(fx::plan_gemm(d, prec, fx::knobs(), 0, P));
  out->family = P.family;
  out->a_kind = P.ak;
  out->b_kind = P.bk;
  out->fast = P.fast ? 1 : 0;
  out->np = P.np;
  out->split = P.g.split;
  out->kt_per_split = P.g.kt_per_split;
  out->tiles_x = P.g.tiles_x;
  out->tiles_y = P.g.tiles_y;
  out->grid_x = (int)P.grid.x;
  out->grid_y = (int)P.grid.y;
  out->grid_z = (int)P.grid.z;
  out->block = (int)P.block.x;
  out->in_launch_reduce = P.counters > 0 ? 1 : 0;
  out->xcd_planes = P.g.xcd_planes;
  out->row_perm = P.g.row_perm;
  out->group_m = P.g.group_m;
  out->persist = P.g.persist;
  return FX_OK;
}

int fx_set_stream_precision(void* stream, int prec) {
  FX_REQUIRE(prec == FX_PREC_DEFAULT || fx::valid_precision(prec),
             "gemm precision: FX_PREC_DEFAULT, FX_PREC_F32, FX_PREC_BF16, FX_PREC_F32S or FX_PREC_F32S2");
  std::lock_guard<std::mutex> lk(fx::g_prec_mu);
  const hipStream_t s = (hipStream_t)stream;
  auto& v = fx::g_prec;
  for (auto it = v.begin(); it != v.end(); ++it)
    if (it->first == s) {
      v.erase(it);
      break;
    }
  if (prec != FX_PREC_DEFAULT) v.emplace_back(s, prec);
  fx::g_prec_any.store(v.empty() ? 0 : 1, std::memory_order_release);
  return FX_OK;
}

int fx_get_stream_precision(void* stream) { return fx::stream_precision((hipStream_t)stream); }

int fx_stream_precision_explicit(void* stream) {
  std::lock_guard<std::mutex> lk(fx::g_prec_mu);
  for (const auto& e : fx::g_prec)
    if (e.first == (hipStream_t)stream) return e.second;
  return FX_PREC_DEFAULT;
}

int fx_set_default_precision(int prec) {
  FX_REQUIRE(fx::valid_precision(prec), "default gemm precision: FX_PREC_F32, FX_PREC_BF16, FX_PREC_F32S or FX_PREC_F32S2");
  fx::g_prec_default.store(prec, std::memory_order_relaxed);
  return FX_OK;
}

int fx_get_default_precision(void) { return fx::g_prec_default.load(std::memory_order_relaxed); }

}  // extern "C"
