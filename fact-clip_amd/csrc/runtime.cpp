// Library runtime shared by every translation unit: the error state, the knob table, the profiler, the
// grid-barrier spin bounds, and the side / aux stream pool with its fork / join helpers (SideLane, ops.h).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "fx_common.h"
#include "ops.h"

namespace fx {

// ---- error state ------------------------------------------------------------
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// ---- profiling (opt-in diagnostic used by bench.py) ---------------------------
namespace {
struct ProfState {
  int max_events = 0;
  std::vector<hipEvent_t> ev;
  std::vector<double> flops, bytes;
  std::vector<int> launches;   // launches an event pair brackets (back-to-back chains: one pair)
  int used = 0;
  // kernel-time pairs (hipExtLaunchKernel) of the kernels launched inside this kind's brackets
  std::vector<hipEvent_t> kev;
  int kused = 0;
  int kdropped = 0;            // kernels launched in a bracket after the pool ran out (not timed)
  hipStream_t open_stream = nullptr;
};
constexpr int kProfKinds = 16;  // 0 conv GEMM, 1 / 2 attention over T fwd / bwd, 3-6 X2Y cores of frame-level
                                // calls (a2f fwd, a2f bwd, f2a fwd, f2a bwd), 7 fused MS-TCN layer, 8 persistent
                                // token-kernel launches (tokdec.hip), 9 SCA frame-memory K/V projection GEMM,
                                // 10 X2Y input projections (k, v, q), 11-14 X2Y cores of segment-level calls,
                                // 15 fused MS-TCN++ layer
std::mutex g_prof_mu;
ProfState g_prof[kProfKinds];
std::atomic<int> g_spin_override[2] = {{-1}, {-1}};   // fx_debug_set_spin: 0 token kernel, 1 X2Y f2a backward

void prof_reset(ProfState& p) {
  for (auto& e : p.ev) (void)hipEventDestroy(e);
  for (auto& e : p.kev) (void)hipEventDestroy(e);
  p = ProfState{};
}
}  // namespace

thread_local int g_prof_open = -1;

void prof_begin(int kind, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (kind < 0 || kind >= kProfKinds) return;
  ProfState& p = g_prof[kind];
  if (p.used >= p.max_events) return;
  (void)hipEventRecord(p.ev[2 * p.used], s);
  p.open_stream = s;
  g_prof_open = kind;
}

void prof_end(int kind, hipStream_t s, double flops, double bytes, int launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (kind < 0 || kind >= kProfKinds) return;
  if (g_prof_open == kind) g_prof_open = -1;
  ProfState& p = g_prof[kind];
  if (p.used >= p.max_events) return;
  (void)hipEventRecord(p.ev[2 * p.used + 1], s);
  p.flops[p.used] = flops;
  p.bytes[p.used] = bytes;
  p.launches[p.used] = launches;
  p.used++;
}

bool prof_kernel_events(hipStream_t s, hipEvent_t* e0, hipEvent_t* e1) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int kind = g_prof_open;
  if (kind < 0 || kind >= kProfKinds) return false;
  ProfState& p = g_prof[kind];
  if (s != p.open_stream) return false;   // (side / aux stream work launched from inside the call)
  if (2 * (size_t)(p.kused + 1) > p.kev.size()) {
    p.kdropped++;
    return false;
  }
  *e0 = p.kev[2 * p.kused];
  *e1 = p.kev[2 * p.kused + 1];
  p.kused++;
  return true;
}

unsigned tok_spin_max() {
  const int o = g_spin_override[0].load(std::memory_order_relaxed);
  if (o > 0) return (unsigned)o;
  return knobs().tok_spin > 0 ? (unsigned)knobs().tok_spin : (1u << 20);
}

unsigned x2y_spin_max() {
  const int o = g_spin_override[1].load(std::memory_order_relaxed);
  return o > 0 ? (unsigned)o : (1u << 22);
}

int coresident_blocks(const void* kernel, int threads, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, int, size_t>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(dev, kernel, threads, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const int n = std::max(per_cu, 0) * std::max(cus, 0);
  cache[key] = n;
  return n;
}

const Knobs& knobs() {
  static Knobs k;
  static std::once_flag once;
  std::call_once(once, [] {
    auto env = [](const char* n) -> const char* { return std::getenv(n); };
    if (const char* p = env("FX_GEMM_PATH")) k.gemm_path = std::string(p) == "tiled" ? 1 : std::string(p) == "direct" ? 2 : 0;
    if (const char* p = env("FX_GEMM_WIDE")) k.gemm_wide = p[0] == '1' ? 1 : 0;
    if (const char* p = env("FX_GEMM_XCDPLANES")) k.gemm_xcd_planes = p[0] != '0';
    if (const char* p = env("FX_GEMM_GROUP")) k.gemm_group = p[0] != '0';
    if (const char* p = env("FX_GEMM_KTAIL")) k.gemm_ktail = p[0] != '0';
    if (const char* p = env("FX_DEC_TOK")) k.dec_tok = p[0] != '0';
    if (const char* p = env("FX_TOK_SPIN")) k.tok_spin = std::max(0, std::atoi(p));
    if (const char* p = env("FX_SIDE_STREAM")) k.side_stream = p[0] != '0';
    if (const char* p = env("FX_MSTCN_DEFER")) k.mstcn_defer = p[0] != '0';
    if (const char* p = env("FX_GEMM_ROWPERM")) k.gemm_row_perm = p[0] != '0';
    if (const char* p = env("FX_GEMM_GROUPM")) k.gemm_group_m = p[0] != '0';
    if (const char* p = env("FX_GEMM_PERSIST")) k.gemm_persist = p[0] != '0';
    if (const char* p = env("FX_FRL_XCD")) k.frl_xcd = std::atoi(p);
    if (const char* p = env("FX_FRL_PAIR")) k.frl_pair = p[0] != '0';
    if (const char* p = env("FX_FRL_MIN_FILL")) k.frl_min_fill = std::atoi(p);
    if (const char* p = env("FX_FRL2_MIN_FILL")) k.frl2_min_fill = std::atoi(p);
    if (const char* p = env("FX_AUX_STREAM")) k.aux_stream = p[0] != '0';
    if (const char* p = env("FX_GRU_POLL2")) k.gru_poll2 = p[0] != '0';
    if (const char* p = env("FX_GRU_STORE_WAVE")) k.gru_store_wave = std::max(0, std::min(2, std::atoi(p)));
    if (const char* p = env("FX_X2Y_A2F_DW")) k.x2y_a2f_dw = p[0] != '0';
    if (const char* p = env("FX_X2Y_FUSED")) k.x2y_fused = p[0] != '0';
    if (const char* p = env("FX_X2Y_F2A_BWD")) k.x2y_f2a_bwd = std::atoi(p);
    if (const char* p = env("FX_X2Y_F2A_ONE")) k.x2y_f2a_one = p[0] != '0';
  });
  return k;
}

// ---- side stream for overlapping independent GEMMs (one per device, created on first use) ----
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t to_side[3] = {};
  hipEvent_t layer_done[4] = {};
  hipEvent_t join = nullptr;
  // a second, short-lived helper stream for work whose result the caller's stream needs before the
  // entry point returns (no backlog of deferred weight gradients in front of it)
  hipStream_t aux = nullptr;
  hipEvent_t aux_fork = nullptr, aux_done = nullptr;
};

static SideStream* side_stream() {
  if (!knobs().side_stream) return nullptr;   // FX_SIDE_STREAM=0: everything on the caller's stream
  static std::mutex mu;
  static std::map<int, SideStream*> pool;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = pool.find(dev);
  if (it != pool.end()) return it->second;
  SideStream* ss = new SideStream();
  // normal priority (the side stream at low priority measured slower: round 3).  FX_SIDE_PRIO_BUILD (a
  // diagnostic build define, -1 low / 1 high) builds the other priorities for A/B runs
#ifndef FX_SIDE_PRIO_BUILD
#define FX_SIDE_PRIO_BUILD 0
#endif
  int prio = 0, least = 0, greatest = 0;
  if (FX_SIDE_PRIO_BUILD != 0 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
    prio = FX_SIDE_PRIO_BUILD < 0 ? least : greatest;
  bool ok = hipStreamCreateWithPriority(&ss->s, hipStreamNonBlocking, prio) == hipSuccess;
  for (auto& e : ss->to_side) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  for (auto& e : ss->layer_done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ss->join, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipStreamCreateWithPriority(&ss->aux, hipStreamNonBlocking, prio) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ss->aux_fork, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ss->aux_done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    delete ss;   // (a partially created set leaks its handles; the caller falls back to one stream)
    return nullptr;
  }
  pool[dev] = ss;
  return ss;
}

SideLane side_lane(hipStream_t main, bool on) {
  SideStream* ss = on ? side_stream() : nullptr;
  return SideLane{main, ss ? ss->s : main, ss};
}

int SideLane::fork(int e) const {
  if (!ss) return FX_OK;
  FX_CHECK_HIP(hipEventRecord(ss->to_side[e], main));
  FX_CHECK_HIP(hipStreamWaitEvent(side, ss->to_side[e], 0));
  return FX_OK;
}

int SideLane::done(int i) const {
  if (!ss) return FX_OK;
  FX_CHECK_HIP(hipEventRecord(ss->layer_done[i & 3], side));
  return FX_OK;
}

int SideLane::wait(int i) const {
  if (!ss) return FX_OK;
  FX_CHECK_HIP(hipStreamWaitEvent(main, ss->layer_done[i & 3], 0));
  return FX_OK;
}

int SideLane::join(bool deferred) const {
  if (!ss || deferred) return FX_OK;
  FX_CHECK_HIP(hipEventRecord(ss->join, side));
  FX_CHECK_HIP(hipStreamWaitEvent(main, ss->join, 0));
  return FX_OK;
}

hipStream_t side_fork(hipStream_t s, int e) {
  const SideLane lane = side_lane(s);
  return lane.fork(e) == FX_OK ? lane.side : s;
}

int side_join_into(hipStream_t s) { return side_lane(s).join(false); }

hipStream_t aux_fork(hipStream_t s) {
  SideStream* ss = side_stream();
  if (!ss || !knobs().aux_stream) return s;   // FX_AUX_STREAM=0: everything on the caller's stream (A/B)
  if (hipEventRecord(ss->aux_fork, s) != hipSuccess || hipStreamWaitEvent(ss->aux, ss->aux_fork, 0) != hipSuccess)
    return s;
  return ss->aux;
}

int aux_join_into(hipStream_t s, hipStream_t a) {
  SideStream* ss = side_stream();
  if (!ss || a == s) return FX_OK;
  FX_CHECK_HIP(hipEventRecord(ss->aux_done, ss->aux));
  FX_CHECK_HIP(hipStreamWaitEvent(s, ss->aux_done, 0));
  return FX_OK;
}
}  // namespace fx

using namespace fx;

extern "C" {

int fx_version(void) { return FX_ABI_VERSION; }

const char* fx_last_error(void) { return g_last_error.c_str(); }

long long fx_struct_size(int which) {
  switch (which) {
    case 0: return (long long)sizeof(fx_gemm_desc);
    case 1: return (long long)sizeof(fx_decoder_params);
    case 2: return (long long)sizeof(fx_mstcn_params);
    case 3: return (long long)sizeof(fx_loss_term);
    case 4: return (long long)sizeof(fx_video_attn);
    case 5: return (long long)sizeof(fx_mstcn2_params);
    case 6: return (long long)sizeof(fx_vn_term);
    case 7: return (long long)sizeof(fx_vn_video);
    case 8: return (long long)sizeof(fx_gemm_plan_info);
    default: return -1;
  }
}

void* fx_side_stream(void) {
  SideStream* ss = side_stream();
  return ss ? (void*)ss->s : nullptr;
}

int fx_side_join(void* stream) {
  const SideLane lane = side_lane((hipStream_t)stream);
  FX_REQUIRE(lane.ss, "side stream unavailable");
  return lane.join(false);
}

// ---------------------------------------------------------------- profiling
int fx_prof_enable(int kind, int max_events) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  FX_REQUIRE(kind >= 0 && kind < kProfKinds && max_events >= 0, "prof: kind out of range");
  ProfState& p = g_prof[kind];
  prof_reset(p);
  p.ev.resize(2 * (size_t)max_events);
  for (auto& e : p.ev) FX_CHECK_HIP(hipEventCreate(&e));
  // kernel-time pairs for the attention-over-T and X2Y kinds (a few kernels per call); the MFMA-bound kinds
  // (conv GEMM, fused layer chains, projection GEMMs) are timed by their brackets alone: their kernels run
  // back to back inside one C call, and an event pair per kernel would add its own dispatch gap to the chain
  const bool kpairs = (kind >= 1 && kind <= 6) || (kind >= 11 && kind <= 14);
  p.kev.resize(kpairs ? 2 * (size_t)max_events * 4 : 0);
  for (auto& e : p.kev) FX_CHECK_HIP(hipEventCreate(&e));
  p.flops.assign(max_events, 0.0);
  p.bytes.assign(max_events, 0.0);
  p.launches.assign(max_events, 0);
  p.max_events = max_events;
  return FX_OK;
}

int fx_prof_collect(int kind, double* total_ms, double* total_flops, double* total_bytes, int* count) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  FX_REQUIRE(kind >= 0 && kind < kProfKinds && g_prof[kind].max_events > 0, "prof: kind not enabled");
  const ProfState& p = g_prof[kind];
  double ms = 0, fl = 0, by = 0;
  int n = 0;
  for (int i = 0; i < p.used; ++i) {
    FX_CHECK_HIP(hipEventSynchronize(p.ev[2 * i + 1]));
    float t = 0.f;
    FX_CHECK_HIP(hipEventElapsedTime(&t, p.ev[2 * i], p.ev[2 * i + 1]));
    ms += t;
    fl += p.flops[i];
    by += p.bytes[i];
    n += p.launches[i];
  }
  *total_ms = ms;
  *total_flops = fl;
  *total_bytes = by;
  *count = n;
  return FX_OK;
}

int fx_prof_collect_kernels(int kind, double* kernel_ms, int* kernels, int* untimed) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  FX_REQUIRE(kind >= 0 && kind < kProfKinds && g_prof[kind].max_events > 0, "prof: kind not enabled");
  const ProfState& p = g_prof[kind];
  double ms = 0;
  for (int i = 0; i < p.kused; ++i) {
    FX_CHECK_HIP(hipEventSynchronize(p.kev[2 * i + 1]));
    float t = 0.f;
    FX_CHECK_HIP(hipEventElapsedTime(&t, p.kev[2 * i], p.kev[2 * i + 1]));
    ms += t;
  }
  *kernel_ms = ms;
  *kernels = p.kused;
  *untimed = p.kdropped;
  return FX_OK;
}

void fx_prof_disable(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& p : g_prof) prof_reset(p);
  g_prof_open = -1;
}

int fx_debug_set_spin(int which, int polls) {
  FX_REQUIRE(which == 0 || which == 1, "fx_debug_set_spin: which is 0 (token kernel) or 1 (X2Y f2a backward)");
  g_spin_override[which].store(polls > 0 ? polls : -1, std::memory_order_relaxed);
  return FX_OK;
}

}  // extern "C"
