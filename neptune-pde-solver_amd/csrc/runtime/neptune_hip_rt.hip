// neptune_hip_rt.hip -- implementation of include/neptune_hip.h: the thin C-ABI runtime the
// emitted host code, the Python frontend and the bench call into.  gfx950 only.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
//   -ffp-contract=off is part of the contract: the reference evaluates body ops one by one in
//   strict IEEE with no FMA (lib/Pipeline/NeptuneIRPassesPipeline.cpp:28-46 has no fusing
//   pass; lib/Compiler/NeptuneCompiler.cpp:332-337 targets cpu "generic"), and parity with
//   it is bit-exact only if the device code does the same.
#define NEPTUNE_HIP_FULL_VARIANTS 1
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"
#include "../kernels/reduce_launch.hpp"
#include "../kernels/util_kernels.hpp"
#include "rt_bodies.hpp"
#include "solver_host.hpp"   // ensure_init and step_loop_destroy_graphs (declared there), stream_capturing

using namespace neptune_hip;

namespace {

struct RuntimeState {
  std::mutex mu;
  bool inited = false;
  int device = -1;
  char arch[256] = "unknown";
  int cus = 0;
  unsigned long long* counter = nullptr;  // device word for count_mismatch
  void* reduce_ws = nullptr;              // kReduceBlocks partials + 1 result (8 B each)
  void* monitor_ws = nullptr;             // partials of one monitored launch (neptune_hip_monitor_workspace), grown on demand
  size_t monitor_bytes = 0;
  // idle device blocks kept for the temporaries of lowered functions (neptune_hip_pool_*)
  struct PoolBlock { void* p; size_t bytes; };
  std::vector<PoolBlock> pool;
  size_t pool_bytes = 0;
  long long pool_cap = -1;                // bytes the pool may hold; -1 = not yet decided
};
RuntimeState& rt() {
  static RuntimeState s;
  return s;
}

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "[NeptuneRT][HIP] %s\n", what);
  abort();
}

inline hipStream_t as_stream(void* p) { return reinterpret_cast<hipStream_t>(p); }

// the built-in bodies live in their own translation units (rt_body_*.hip)
const rtbody::Entry* body_entry(int body) {
  switch (body) {
    case NEPTUNE_HIP_BODY_LAP2D5_F64: return &rtbody::lap2d5();
    case NEPTUNE_HIP_BODY_LAP3D7_F64: return &rtbody::lap3d7();
    case NEPTUNE_HIP_BODY_LAP3D27_F32: return &rtbody::lap3d27();
    case NEPTUNE_HIP_BODY_LAP1D3_F64: return &rtbody::lap1d3();
  }
  return nullptr;
}

size_t body_elem_size(int body) { return body == NEPTUNE_HIP_BODY_LAP3D27_F32 ? 4 : 8; }

}  // namespace

namespace {
// average milliseconds per launch of `launch(cfg)` on `st` (HIP events; blocking); negative = the launch's error code
template <class L>
double time_launches(L&& launch, hipStream_t st, const neptune_hip_launch_cfg_t* cfg, int warmup, int reps) {
  if (reps <= 0) return -1.0;
  for (int i = 0; i < warmup; ++i) {
    const int rc = launch(cfg);
    if (rc != NEPTUNE_HIP_OK) return (double)rc;
  }
  hipEvent_t e0, e1;
  NEPTUNE_HIP_CHECK(hipEventCreate(&e0));
  NEPTUNE_HIP_CHECK(hipEventCreate(&e1));
  NEPTUNE_HIP_CHECK(hipEventRecord(e0, st));
  int rc = NEPTUNE_HIP_OK;
  for (int i = 0; i < reps && rc == NEPTUNE_HIP_OK; ++i) rc = launch(cfg);
  NEPTUNE_HIP_CHECK(hipEventRecord(e1, st));
  NEPTUNE_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  NEPTUNE_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  NEPTUNE_HIP_CHECK(hipEventDestroy(e0));
  NEPTUNE_HIP_CHECK(hipEventDestroy(e1));
  return rc != NEPTUNE_HIP_OK ? (double)rc : (double)ms / reps;
}

// Plan-time tuning shared by the built-in bodies and lowered applies: the automatic launch first, then every
// march tile `nv` the code object behind `launch` holds x a few chunk lengths.  All candidates compute the same
// bits, so the timed launches leave `out` exactly as a normal launch would.
// Two passes: every candidate once (reps launches), then a play-off of the four fastest, measured again in turn with
// three times the repetitions -- the first pass runs while the clocks are still settling (candidates measured late look
// faster than they are: a 27-point workload once picked the last tile of the list at 0.189 ms and then ran at 0.199),
// the play-off compares like with like.
template <class L>
int autotune_launches(L&& launch, bool march_planned, int rank, int nv, hipStream_t st, int reps,
                      neptune_hip_launch_cfg_t* best, double* best_ms) {
  if (reps <= 0) reps = 5;
  neptune_hip_launch_cfg_t probe = {NEPTUNE_HIP_KERNEL_AUTO, -1, 0, 0};
  *best = probe;
  double best_t = time_launches(launch, st, &probe, 2, reps);
  if (best_t < 0) return (int)best_t;
  // short launches need more repetitions to tell tiles 2-3 % apart: at least ~4 ms of launches per candidate
  if (best_t > 0 && best_t * reps < 4.0) reps = (int)(4.0 / best_t) + 1 < 24 ? (int)(4.0 / best_t) + 1 : 24;
  struct Cand { neptune_hip_launch_cfg_t cfg; double t; };
  std::vector<Cand> cands;
  cands.push_back({probe, best_t});
  if (march_planned) {
    const int chunks3[] = {0, 32, 64, 128, 256, 512}, chunks2[] = {0};
    for (int v = 0; v < nv; ++v) {
      const MarchVariant* mv = march_variant(rank, v);   // indices below the caller's count name the same tiles everywhere
      if (!mv) break;
      const bool tile2 = rank == 2 && mv->jk;
      const int* chunks = (rank == 3 || !tile2) ? chunks3 : chunks2;
      const int nc = (rank == 3 || !tile2) ? 6 : 1;
      for (int c = 0; c < nc; ++c) {
        neptune_hip_launch_cfg_t cfg = {NEPTUNE_HIP_KERNEL_MARCH, v, chunks[c], 0};
        const double t = time_launches(launch, st, &cfg, 1, reps);
        if (t > 0) cands.push_back({cfg, t});
      }
    }
    std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.t < b.t; });
    const size_t top = cands.size() < 4 ? cands.size() : 4;
    for (size_t i = 0; i < top; ++i) cands[i].t = 1e30;
    for (int round = 0; round < 2; ++round)
      for (size_t i = 0; i < top; ++i) {
        const double t = time_launches(launch, st, &cands[i].cfg, 1, 3 * reps);
        if (t > 0 && t < cands[i].t) cands[i].t = t;
      }
    size_t win = 0;
    for (size_t i = 1; i < top; ++i)
      if (cands[i].t < cands[win].t) win = i;
    *best = cands[win].cfg;
    best_t = cands[win].t;
  }
  if (best_ms) *best_ms = best_t;
  return NEPTUNE_HIP_OK;
}
}  // namespace


namespace {
template <bool XPAY>
int vec_update(int dtype, int64_t n, double a, const void* x, void* y, void* stream) {
  if (!x || !y || n < 0) return NEPTUNE_HIP_EINVAL;
  if (n == 0) return NEPTUNE_HIP_OK;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  // the kernel reads x and writes y through __restrict__ pointers: overlapping ranges would be undefined behaviour
  if (buffers_overlap(x, (size_t)n * (dtype == NEPTUNE_HIP_F64 ? 8 : 4), y, (size_t)n * (dtype == NEPTUNE_HIP_F64 ? 8 : 4))) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const FlatGrid fg = flat_grid(n, dtype == NEPTUNE_HIP_F64 ? 8 : 4, {x, y});
  if (dtype == NEPTUNE_HIP_F64)
    flat_launch(fg, as_stream(stream), neptune_vec_update<double, XPAY, true>, neptune_vec_update<double, XPAY, false>, n, a, x, y);
  else
    flat_launch(fg, as_stream(stream), neptune_vec_update<float, XPAY, true>, neptune_vec_update<float, XPAY, false>, n, a, x, y);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  return NEPTUNE_HIP_OK;
}
}  // namespace

namespace {
// (a - b) * (a - b): the term of S, as a two-input pointwise body for the reduce(apply) kernels
template <class T>
struct DiffSquared {
  template <class A>
  __device__ __forceinline__ T operator()(const A& acc) const {
    const T d = acc.template get<0, 0, 0, 0>() - acc.template get<1, 0, 0, 0>();
    return d * d;
  }
};
// a * b: the term of a dot product (one rounding), likewise
template <class T>
struct Product {
  template <class A>
  __device__ __forceinline__ T operator()(const A& acc) const { return acc.template get<0, 0, 0, 0>() * acc.template get<1, 0, 0, 0>(); }
};
// sum over apply.bounds x launch region of `g` of Term(a, b), in one read-only pass: a = a field in the result's box, b = one
// in input 0's box
template <class T, class Term>
int two_field_sum(const neptune_hip_apply_geom_t* g, const void* a, const void* b, void* sum_out, hipStream_t st) {
  // a two-input apply geometry: input 0 = a in the result's box, input 1 = b in input 0's box; reduced box = bounds x region
  neptune_hip_apply_geom_t g2 = *g;
  g2.num_inputs = 2;
  bool empty = false;
  for (int d = 0; d < g->rank; ++d) {
    g2.in_lb[0][d] = g->out_lb[d]; g2.in_ub[0][d] = g->out_ub[d];
    g2.in_lb[1][d] = g->in_lb[0][d]; g2.in_ub[1][d] = g->in_ub[0][d];
    const int64_t lo = std::max(g->lb[d] - g->out_lb[d], g->region_lb[d]), hi = std::min(g->ub[d] - g->out_lb[d], g->region_ub[d]);
    g2.region_lb[d] = lo;
    g2.region_ub[d] = hi;
    empty = empty || lo >= hi;
  }
  if (empty || geom_bounds_empty(g)) {
    NEPTUNE_HIP_CHECK(hipMemsetAsync(sum_out, 0, sizeof(T), st));   // +0
    return NEPTUNE_HIP_OK;
  }
  const void* ptrs[2] = {a, b};
  DirectParams<T, 2> P{};
  switch (g->rank) {   // the kernels below are the rank-3 instantiations: absent axes have extent 1
    case 1: fill_direct_params<T, 1, 2>(&g2, ptrs, nullptr, P); break;
    case 2: fill_direct_params<T, 2, 2>(&g2, ptrs, nullptr, P); break;
    default: fill_direct_params<T, 3, 2>(&g2, ptrs, nullptr, P); break;
  }
  const ReduceApplyPlan pl = plan_reduce_apply(P, ptrs, true);
  if (!pl.narrow) return NEPTUNE_HIP_EUNSUPPORTED;   // the kernels keep coordinates and row indices in 32 bits
  launch_reduce_apply<RedSum<T>, RedSum<T>, true, Term, T, 3, 2>(pl, P, Term{}, static_cast<T*>(rt().reduce_ws),
                                                                  static_cast<T*>(sum_out), st);
  return NEPTUNE_HIP_OK;
}
template <class T>
int update_norm(const neptune_hip_apply_geom_t* g, const void* a, const void* b, void* sum_out, hipStream_t st) {
  return two_field_sum<T, DiffSquared<T>>(g, a, b, sum_out, st);
}
}  // namespace

// ---- neptune_ir.reduce: the plan and the launch behind neptune_hip_reduce
namespace {
// per-rank arrays -> the kernels' (I,J,K) order; absent axes take `f`
void to_axes3(int rank, const int64_t* a, int64_t* o, int64_t f) {
  o[0] = o[1] = o[2] = f;
  if (rank == 3) { o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; }
  else if (rank == 2) { o[0] = a[0]; o[2] = a[1]; }
  else { o[2] = a[0]; }
}
// the checks and the launch geometry every kind shares: which first-pass kernel, how many workgroups, the box
struct ReducePlan {
  bool whole;
  int blocks;
  int64_t total, count;   // cells of the reduced box, cells of the buffer
  ReduceBoxParams P;
};
int reduce_plan(int dtype, int rank, const void* src, const int64_t* src_lb, const int64_t* src_ub, const int64_t* lb,
                const int64_t* ub, const double* result, ReducePlan& pl) {
  if (!src || !src_lb || !src_ub || !result) return NEPTUNE_HIP_EINVAL;
  if (rank < 1 || rank > kMaxRank) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  int64_t ext[3], off[3], shp[3];
  bool whole = true;
  int64_t total = 1, count = 1;
  for (int d = 0; d < rank; ++d) {
    shp[d] = src_ub[d] - src_lb[d];
    if (shp[d] <= 0) return NEPTUNE_HIP_EINVAL;
    const int64_t l = lb ? lb[d] : src_lb[d], u = ub ? ub[d] : src_ub[d];
    ext[d] = u - l;
    off[d] = l - src_lb[d];
    if (ext[d] < 0) return NEPTUNE_HIP_EINVAL;
    if (ext[d] > 0 && (off[d] < 0 || off[d] + ext[d] > shp[d])) return NEPTUNE_HIP_EOOB;  // memref.load out of range
    whole = whole && off[d] == 0 && ext[d] == shp[d] && ((uintptr_t)src % 16 == 0);
    total *= ext[d];
    count *= shp[d];
  }
  int blocks = (int)((total + 255) / 256 < kReduceBlocks ? (total + 255) / 256 : kReduceBlocks);
  if (!whole) {  // box kernel: one unit of work = 4 row chunks of 256 lanes x 16 bytes
    const int64_t cells = 256 * (dtype == NEPTUNE_HIP_F64 ? 2 : 4);
    const int64_t last = ext[rank - 1];
    const int64_t trips = ((total / (last ? last : 1)) * ((last + cells - 1) / cells) + 3) / 4;
    blocks = (int)(trips < kReduceBlocks ? (trips < 1 ? 1 : trips) : kReduceBlocks);
  }
  to_axes3(rank, ext, pl.P.ext, 1);
  to_axes3(rank, off, pl.P.off, 0);
  to_axes3(rank, shp, pl.P.shape, 1);
  pl.whole = whole;
  pl.blocks = blocks;
  pl.total = total;
  pl.count = count;
  return NEPTUNE_HIP_OK;
}

// the first pass on POp, the root on FOp (POp's combine, the identity map, the kind's finish), the result read back
template <class T, class POp, class FOp>
int reduce_launch(const ReducePlan& pl, const void* src, double* result, hipStream_t st) {
  T* part = static_cast<T*>(rt().reduce_ws);
  if (pl.whole) hipLaunchKernelGGL((neptune_reduce_partial_flat<T, POp>), dim3(pl.blocks), dim3(256), 0, st, (const T*)src, pl.count, part);
  else hipLaunchKernelGGL((neptune_reduce_partial_box<T, POp>), dim3(pl.blocks), dim3(256), 0, st, (const T*)src, pl.P, part);
  launch_reduce_root<T, FOp>(part, pl.blocks, part + kReduceBlocks, st);
  *result = read_back(part + kReduceBlocks, st);
  return NEPTUNE_HIP_OK;
}
// kind / raw -> the ops of the kind table (ReduceOps, util_kernels.hpp)
template <class T, int KIND, bool RAW = false>
int reduce_as(const ReducePlan& pl, const void* src, double* result, hipStream_t st) {
  using Ops = ReduceOps<KIND, T, RAW>;
  return reduce_launch<T, typename Ops::POp, typename Ops::FOp>(pl, src, result, st);
}
template <class T>
int reduce_kind(int kind, bool raw, const ReducePlan& pl, const void* src, double* result, hipStream_t st) {
  switch (kind) {
    case NEPTUNE_HIP_REDUCE_SUM: return reduce_as<T, NEPTUNE_HIP_REDUCE_SUM>(pl, src, result, st);
    case NEPTUNE_HIP_REDUCE_MAX: return reduce_as<T, NEPTUNE_HIP_REDUCE_MAX>(pl, src, result, st);
    case NEPTUNE_HIP_REDUCE_MIN: return reduce_as<T, NEPTUNE_HIP_REDUCE_MIN>(pl, src, result, st);
    case NEPTUNE_HIP_REDUCE_L1: return reduce_as<T, NEPTUNE_HIP_REDUCE_L1>(pl, src, result, st);
    default: break;
  }
  return raw ? reduce_as<T, NEPTUNE_HIP_REDUCE_L2, true>(pl, src, result, st) : reduce_as<T, NEPTUNE_HIP_REDUCE_L2>(pl, src, result, st);
}
}  // namespace

// solver_host.hpp: the runtime is up from here on -- on device 0 unless neptune_hip_init has chosen another
void neptune_hip::ensure_init() {
  RuntimeState& s = rt();
  if (s.inited) return;
  neptune_hip_init(s.device < 0 ? 0 : s.device);
}

extern "C" {

// ---------------------------------------------------------------- runtime
void neptune_hip_init(int device) {
  RuntimeState& s = rt();
  std::lock_guard<std::mutex> lk(s.mu);
  if (s.inited && s.device == device) return;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) die("no HIP device available");
  if (device < 0 || device >= count) die("neptune_hip_init: device index out of range");
  NEPTUNE_HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  NEPTUNE_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  strncpy(s.arch, prop.gcnArchName, sizeof(s.arch) - 1);
  s.cus = prop.multiProcessorCount;
  if (strncmp(s.arch, "gfx950", 6) != 0)
    fprintf(stderr, "[NeptuneRT][HIP] warning: built for gfx950, device reports %s\n", s.arch);
  if (!s.counter) NEPTUNE_HIP_CHECK(hipMalloc((void**)&s.counter, sizeof(unsigned long long)));
  if (!s.reduce_ws) NEPTUNE_HIP_CHECK(hipMalloc(&s.reduce_ws, (kReduceBlocks + 1) * 8));
  s.device = device;
  s.inited = true;
}

void neptune_hip_finalize(void) {
  RuntimeState& s = rt();
  std::lock_guard<std::mutex> lk(s.mu);
  if (!s.inited) return;
  if (s.counter) {
    (void)hipFree(s.counter);
    s.counter = nullptr;
  }
  if (s.reduce_ws) {
    (void)hipFree(s.reduce_ws);
    s.reduce_ws = nullptr;
  }
  if (s.monitor_ws) {
    (void)hipFree(s.monitor_ws);
    s.monitor_ws = nullptr;
    s.monitor_bytes = 0;
  }
  step_loop_destroy_graphs();
  for (auto& b : s.pool) (void)hipFree(b.p);
  s.pool.clear();
  s.pool_bytes = 0;
  s.inited = false;
}

int neptune_hip_available(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count > 0 ? 1 : 0;
}

const char* neptune_hip_arch(void) {
  ensure_init();
  return rt().arch;
}
int neptune_hip_cu_count(void) {
  ensure_init();
  return rt().cus;
}
const char* neptune_hip_version(void) { return "neptune-hip 0.1 (gfx950, ffp-contract=off)"; }

void* neptune_hip_malloc(size_t bytes) {
  ensure_init();
  void* p = nullptr;
  if (bytes == 0) bytes = 16;
  NEPTUNE_HIP_CHECK(hipMalloc(&p, bytes));
  return p;
}
void neptune_hip_free(void* dptr) {
  if (dptr) NEPTUNE_HIP_CHECK(hipFree(dptr));
}
void neptune_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
}
void neptune_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
}
void neptune_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
}
void neptune_hip_stream_sync(void* stream) { NEPTUNE_HIP_CHECK(hipStreamSynchronize(as_stream(stream))); }
void neptune_hip_device_sync(void) { NEPTUNE_HIP_CHECK(hipDeviceSynchronize()); }

int neptune_hip_is_device_ptr(const void* p) {
  if (!p) return 0;
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // plain host memory is reported as an error; clear it
    return 0;
  }
  return attr.type == hipMemoryTypeDevice ? 1 : 0;
}

// ---------------------------------------------------------------- block pool
// hipMalloc/hipFree of a field-sized block costs far more than the kernels that use it (an 8 GiB temp:
// hundreds of milliseconds for mapping and unmapping), and a lowered function needs one for every
// apply result it cannot write straight into a destination field.  Idle blocks are therefore kept and
// handed out again: best fit within 25 % of the request, LIFO among equals.  Blocks are only returned
// by scopes that have synchronised their stream, so a cached block is never in use.
static long long pool_cap_bytes(RuntimeState& s) {
  if (s.pool_cap < 0) {
    const char* e = getenv("NEPTUNE_HIP_POOL_BYTES");
    if (e && *e) {
      s.pool_cap = atoll(e);
    } else {
      size_t fr = 0, tot = 0;
      s.pool_cap = (hipMemGetInfo(&fr, &tot) == hipSuccess) ? (long long)(tot / 4) : (long long)(16ll << 30);
    }
    if (s.pool_cap < 0) s.pool_cap = 0;
  }
  return s.pool_cap;
}

void* neptune_hip_pool_alloc(size_t bytes) {
  ensure_init();
  RuntimeState& s = rt();
  if (bytes == 0) bytes = 16;
  {
    std::lock_guard<std::mutex> lk(s.mu);
    int best = -1;
    for (int i = (int)s.pool.size() - 1; i >= 0; --i) {
      const size_t b = s.pool[i].bytes;
      if (b >= bytes && b - bytes <= bytes / 4 && (best < 0 || b < s.pool[best].bytes)) best = i;
    }
    if (best >= 0) {
      void* p = s.pool[best].p;
      s.pool_bytes -= s.pool[best].bytes;
      s.pool.erase(s.pool.begin() + best);
      return p;
    }
  }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    neptune_hip_pool_trim();  // out of memory with idle blocks held back: give them up and retry once
    NEPTUNE_HIP_CHECK(hipMalloc(&p, bytes));
  }
  return p;
}

void neptune_hip_pool_release(void* p, size_t bytes) {
  if (!p) return;
  RuntimeState& s = rt();
  if (bytes == 0) bytes = 16;
  {
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.inited && (long long)(s.pool_bytes + bytes) <= pool_cap_bytes(s)) {
      s.pool.push_back({p, bytes});
      s.pool_bytes += bytes;
      return;
    }
  }
  NEPTUNE_HIP_CHECK(hipFree(p));
}

void neptune_hip_pool_trim(void) {
  RuntimeState& s = rt();
  std::vector<RuntimeState::PoolBlock> blocks;
  {
    std::lock_guard<std::mutex> lk(s.mu);
    blocks.swap(s.pool);
    s.pool_bytes = 0;
  }
  for (auto& b : blocks) NEPTUNE_HIP_CHECK(hipFree(b.p));
}

size_t neptune_hip_pool_cached_bytes(void) {
  RuntimeState& s = rt();
  std::lock_guard<std::mutex> lk(s.mu);
  return s.pool_bytes;
}

static int64_t g_slab[4] = {0, 0, 0, 0};
static bool g_slab_set = false;
static void* g_slab_pending = nullptr;  // hipEvent_t of a halo exchange still in flight on another stream
int neptune_hip_set_slab(int64_t start, int64_t stop, int64_t ghost_lo, int64_t ghost_hi) {
  if (stop < start || ghost_lo < 0 || ghost_hi < 0) return NEPTUNE_HIP_EINVAL;
  g_slab[0] = start; g_slab[1] = stop; g_slab[2] = ghost_lo; g_slab[3] = ghost_hi;
  g_slab_set = true;
  return NEPTUNE_HIP_OK;
}
int neptune_hip_clear_slab(void) {
  g_slab_set = false;
  g_slab_pending = nullptr;
  return NEPTUNE_HIP_OK;
}
int neptune_hip_set_slab_pending(void* event) {
  if (!g_slab_set) return NEPTUNE_HIP_EINVAL;
  g_slab_pending = event;
  return NEPTUNE_HIP_OK;
}
void* neptune_hip_get_slab_pending(void) { return g_slab_set ? g_slab_pending : nullptr; }
int neptune_hip_get_slab(int64_t out[4]) {
  if (!g_slab_set) return 0;
  for (int i = 0; i < 4; ++i) out[i] = g_slab[i];
  return 1;
}

void neptune_rt_free(void* p) {
  if (!p) return;
  if (neptune_hip_is_device_ptr(p)) NEPTUNE_HIP_CHECK(hipFree(p));
  else free(p);
}

// ---------------------------------------------------------------- apply
int neptune_hip_check_geom(const neptune_hip_apply_geom_t* g,
                           const int32_t radius[NEPTUNE_HIP_MAX_INPUTS][NEPTUNE_HIP_MAX_RANK]) {
  if (!radius) return geom_validate(g);
  return geom_check_radius(g, radius);
}

int neptune_hip_apply_builtin(int body, const neptune_hip_apply_geom_t* g, const void* const* in, void* out,
                              void* stream, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !in || !out) return NEPTUNE_HIP_EINVAL;
  if (body < 0 || body >= NEPTUNE_HIP_BODY_COUNT) return NEPTUNE_HIP_EINVAL;
  int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  for (int k = 0; k < g->num_inputs; ++k)
    if (!in[k]) return NEPTUNE_HIP_EINVAL;
  rc = check_no_alias(g, in, out, body_elem_size(body));
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  return body_entry(body)->apply(g, in, out, as_stream(stream), cfg);
}

// ---------------------------------------------------------------- monitored applies
int neptune_hip_apply_builtin_norm(int body, const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* sum_out,
                                   void* stream, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !in || !out || !sum_out) return NEPTUNE_HIP_EINVAL;
  if (body < 0 || body >= NEPTUNE_HIP_BODY_COUNT) return NEPTUNE_HIP_EINVAL;
  int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  for (int k = 0; k < g->num_inputs; ++k)
    if (!in[k]) return NEPTUNE_HIP_EINVAL;
  rc = check_no_alias(g, in, out, body_elem_size(body));
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  return body_entry(body)->apply_norm(g, in, out, sum_out, as_stream(stream), cfg);
}

// ---------------------------------------------------------------- dot-monitored applies
int neptune_hip_apply_builtin_dot(int body, const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* dot_out,
                                  void* stream, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !in || !out || !dot_out) return NEPTUNE_HIP_EINVAL;
  if (body < 0 || body >= NEPTUNE_HIP_BODY_COUNT) return NEPTUNE_HIP_EINVAL;
  int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  for (int k = 0; k < g->num_inputs; ++k)
    if (!in[k]) return NEPTUNE_HIP_EINVAL;
  rc = check_no_alias(g, in, out, body_elem_size(body));
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  return body_entry(body)->apply_dot(g, in, out, dot_out, as_stream(stream), cfg);
}

int neptune_hip_dot(int dtype, const neptune_hip_apply_geom_t* g, const void* a, const void* b, void* out_dev, void* stream) {
  if (!g || !a || !b || !out_dev) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  const int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  return dtype == NEPTUNE_HIP_F64 ? two_field_sum<double, Product<double>>(g, a, b, out_dev, as_stream(stream))
                                  : two_field_sum<float, Product<float>>(g, a, b, out_dev, as_stream(stream));
}

void* neptune_hip_monitor_workspace(size_t bytes, void* stream) {
  ensure_init();
  RuntimeState& s = rt();
  std::lock_guard<std::mutex> lk(s.mu);
  if (bytes <= s.monitor_bytes) return s.monitor_ws;
  // growing frees the old block, which waits for the launches that may still write it: not inside a stream capture
  if (stream_capturing(stream)) return nullptr;
  size_t want = s.monitor_bytes ? s.monitor_bytes : (size_t)1 << 16;
  while (want < bytes) want *= 2;
  if (s.monitor_ws) NEPTUNE_HIP_CHECK(hipFree(s.monitor_ws));
  s.monitor_ws = nullptr;
  s.monitor_bytes = 0;
  NEPTUNE_HIP_CHECK(hipMalloc(&s.monitor_ws, want));
  s.monitor_bytes = want;
  return s.monitor_ws;
}

int neptune_hip_update_norm(int dtype, const neptune_hip_apply_geom_t* g, const void* a, const void* b, void* sum_out, void* stream) {
  if (!g || !a || !b || !sum_out) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  const int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  return dtype == NEPTUNE_HIP_F64 ? update_norm<double>(g, a, b, sum_out, as_stream(stream)) : update_norm<float>(g, a, b, sum_out, as_stream(stream));
}

// two or three chained applies of a built-in body in one pass over HBM (csrc/kernels/apply_march2.hpp)
int neptune_hip_apply_chain_builtin(int body, int applies, const neptune_hip_apply_geom_t* g, const void* const* in, void* out,
                                    void* stream, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !in || !out) return NEPTUNE_HIP_EINVAL;
  if (body < 0 || body >= NEPTUNE_HIP_BODY_COUNT) return NEPTUNE_HIP_EINVAL;
  if (applies != 2 && applies != 3) return NEPTUNE_HIP_EUNSUPPORTED;
  int rc = geom_validate(g);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (g->num_inputs != 1 || !in[0]) return NEPTUNE_HIP_EUNSUPPORTED;
  rc = check_no_alias(g, in, out, body_elem_size(body));
  if (rc != NEPTUNE_HIP_OK) return rc;
  ensure_init();
  const rtbody::Entry* e = body_entry(body);
  if (!e->chain) return NEPTUNE_HIP_EUNSUPPORTED;   // 1-D and box bodies: one launch per apply
  return e->chain(applies, g, in, out, as_stream(stream), cfg);
}
int neptune_hip_apply2_builtin(int body, const neptune_hip_apply_geom_t* g, const void* const* in, void* out,
                               void* stream, const neptune_hip_launch_cfg_t* cfg) {
  return neptune_hip_apply_chain_builtin(body, 2, g, in, out, stream, cfg);
}

int neptune_hip_apply_builtin_plan(int body, const neptune_hip_apply_geom_t* g, const void* const* in,
                                   const void* out, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !in || !out) return NEPTUNE_HIP_EINVAL;
  const rtbody::Entry* e = body_entry(body);
  return e ? e->plan(g, in, out, cfg) : NEPTUNE_HIP_EINVAL;
}

int neptune_hip_apply_builtin_variant(int body, const neptune_hip_apply_geom_t* g, const neptune_hip_launch_cfg_t* cfg) {
  if (!g) return NEPTUNE_HIP_EINVAL;
  const rtbody::Entry* e = body_entry(body);
  return e ? e->variant(g, cfg) : NEPTUNE_HIP_EINVAL;
}

const char* neptune_hip_kernel_name(int kernel) {
  switch (kernel) {
    case NEPTUNE_HIP_KERNEL_DIRECT: return "neptune_apply_direct";
    case NEPTUNE_HIP_KERNEL_MARCH: return "neptune_apply_march";
  }
  return "";
}
int neptune_hip_march_variant_count(int rank) { return march_variant_count(rank); }
const char* neptune_hip_march_variant_name(int rank, int variant) {
  const MarchVariant* v = march_variant(rank, variant);
  return v ? v->name : "";
}

// ---------------------------------------------------------------- store
int neptune_hip_store_full(int dtype, const void* src, void* dst, int64_t count, void* stream) {
  if (!src || !dst || count < 0) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = (size_t)count * (dtype == NEPTUNE_HIP_F64 ? 8 : 4);
  if (bytes == 0 || src == dst) return NEPTUNE_HIP_OK;
  // 16-byte-aligned device buffers: the streaming copy kernel (one 16-byte load per lane, non-temporal store: 6.4 TB/s on a
  // 1024^3 fp64 field against 5.1 for hipMemcpyAsync, bench.py roofline.copy_ceiling); anything else, and the last few
  // bytes, through the runtime's copy
  const bool aligned = ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
  const int64_t n16 = aligned ? (int64_t)(bytes / 16) : 0;
  if (n16 > 0) {
    ensure_init();
    const int64_t blocks = (n16 + 255) / 256;
    if (blocks <= 0x7fffffffLL) {
      hipLaunchKernelGGL((neptune_copy16_unrolled<1, false, true>), dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream),
                         (const u32x4*)src, (u32x4*)dst, n16);
      NEPTUNE_HIP_CHECK(hipGetLastError());
      const size_t done = (size_t)n16 * 16;
      if (done < bytes)
        NEPTUNE_HIP_CHECK(hipMemcpyAsync((char*)dst + done, (const char*)src + done, bytes - done, hipMemcpyDeviceToDevice, as_stream(stream)));
      return NEPTUNE_HIP_OK;
    }
  }
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
  return NEPTUNE_HIP_OK;
}

int neptune_hip_store_box(int dtype, int rank, const void* src, const int64_t* src_lb, const int64_t* src_ub,
                          void* dst, const int64_t* dst_lb, const int64_t* dst_ub, const int64_t* lb,
                          const int64_t* ub, void* stream) {
  if (!src || !dst || !src_lb || !src_ub || !dst_lb || !dst_ub || !lb || !ub) return NEPTUNE_HIP_EINVAL;
  if (rank < 1 || rank > kMaxRank) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  int64_t ext[3], soff[3], doff[3], ss[3], ds[3];
  for (int d = 0; d < rank; ++d) {
    ext[d] = ub[d] - lb[d];
    soff[d] = lb[d] - src_lb[d];
    doff[d] = lb[d] - dst_lb[d];
    ss[d] = src_ub[d] - src_lb[d];
    ds[d] = dst_ub[d] - dst_lb[d];
    if (ext[d] < 0 || ss[d] <= 0 || ds[d] <= 0) return NEPTUNE_HIP_EINVAL;
    // the subviews of the reference (DataflowLowering.cpp:212-215) must lie inside their buffers
    if (ext[d] > 0 && (soff[d] < 0 || soff[d] + ext[d] > ss[d] || doff[d] < 0 || doff[d] + ext[d] > ds[d]))
      return NEPTUNE_HIP_EOOB;
  }
  BoxCopyParams P;
  to_axes3(rank, ext, P.ext, 1);
  to_axes3(rank, soff, P.soff, 0);
  to_axes3(rank, doff, P.doff, 0);
  to_axes3(rank, ss, P.sshape, 1);
  to_axes3(rank, ds, P.dshape, 1);
  const int64_t total = P.ext[0] * P.ext[1] * P.ext[2];
  if (total == 0) return NEPTUNE_HIP_OK;
  // one workgroup per chunk of 256 lanes x 16 bytes of one row of the box (see the kernel)
  const int64_t chunk_cells = 256 * (dtype == NEPTUNE_HIP_F64 ? 2 : 4);
  const int64_t blocks = P.ext[0] * P.ext[1] * ((P.ext[2] + chunk_cells - 1) / chunk_cells);
  if (blocks > 0x7fffffffLL) return NEPTUNE_HIP_EUNSUPPORTED;
  ensure_init();
  if (dtype == NEPTUNE_HIP_F64)
    hipLaunchKernelGGL(neptune_store_box<double>, grid_for_blocks(blocks), dim3(256), 0, as_stream(stream),
                       (const double*)src, (double*)dst, P);
  else
    hipLaunchKernelGGL(neptune_store_box<float>, grid_for_blocks(blocks), dim3(256), 0, as_stream(stream),
                       (const float*)src, (float*)dst, P);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  return NEPTUNE_HIP_OK;
}

// ---------------------------------------------------------------- reduce
void* neptune_hip_reduce_workspace(void) {
  ensure_init();
  return rt().reduce_ws;
}

int neptune_hip_reduce_sum(int dtype, int rank, const void* src, const int64_t* src_lb, const int64_t* src_ub,
                           const int64_t* lb, const int64_t* ub, double* result, void* stream) {
  return neptune_hip_reduce(NEPTUNE_HIP_REDUCE_SUM, dtype, rank, src, src_lb, src_ub, lb, ub, result, stream);
}

int neptune_hip_reduce(int kind_flags, int dtype, int rank, const void* src, const int64_t* src_lb, const int64_t* src_ub,
                       const int64_t* lb, const int64_t* ub, double* result, void* stream) {
  const bool raw = (kind_flags & NEPTUNE_HIP_REDUCE_RAW) != 0;
  const int kind = kind_flags & ~NEPTUNE_HIP_REDUCE_RAW;
  if (kind < NEPTUNE_HIP_REDUCE_SUM || kind > NEPTUNE_HIP_REDUCE_L2) return NEPTUNE_HIP_EINVAL;
  ReducePlan pl;
  const int rc = reduce_plan(dtype, rank, src, src_lb, src_ub, lb, ub, result, pl);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (pl.total == 0) {  // empty domain: the reference's loop never runs, the accumulator stays at the kind's identity (sum: 0)
    *result = reduce_identity(kind);
    return NEPTUNE_HIP_OK;
  }
  ensure_init();
  hipStream_t st = as_stream(stream);
  return dtype == NEPTUNE_HIP_F64 ? reduce_kind<double>(kind, raw, pl, src, result, st) : reduce_kind<float>(kind, raw, pl, src, result, st);
}

// ---------------------------------------------------------------- Krylov vector updates
int neptune_hip_axpy(int dtype, int64_t n, double a, const void* x, void* y, void* stream) {
  return vec_update<false>(dtype, n, a, x, y, stream);
}
int neptune_hip_xpay(int dtype, int64_t n, const void* x, double a, void* y, void* stream) {
  return vec_update<true>(dtype, n, a, x, y, stream);
}

// ---------------------------------------------------------------- helpers
int neptune_hip_fill_hash(int dtype, void* dst, int64_t count, int64_t index_offset, uint64_t seed,
                          void* stream) {
  if (!dst || count < 0) return NEPTUNE_HIP_EINVAL;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  if (count == 0) return NEPTUNE_HIP_OK;
  ensure_init();
  const int64_t want = (count + 255) / 256;
  const uint32_t blocks = (uint32_t)(want < 8192 ? want : 8192);
  if (dtype == NEPTUNE_HIP_F64)
    hipLaunchKernelGGL(neptune_fill_hash<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (double*)dst,
                       count, index_offset, seed);
  else
    hipLaunchKernelGGL(neptune_fill_hash<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (float*)dst,
                       count, index_offset, seed);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  return NEPTUNE_HIP_OK;
}

double neptune_hip_hash_value(int dtype, int64_t index, uint64_t seed) {
  return dtype == NEPTUNE_HIP_F32 ? (double)hash_f32(index, seed) : hash_f64(index, seed);
}

int64_t neptune_hip_count_mismatch(int dtype, const void* a, const void* b, int64_t count, void* stream) {
  if (!a || !b || count < 0) return -1;
  if (dtype != NEPTUNE_HIP_F64 && dtype != NEPTUNE_HIP_F32) return -1;
  if (count == 0) return 0;
  ensure_init();
  RuntimeState& s = rt();
  hipStream_t st = as_stream(stream);
  NEPTUNE_HIP_CHECK(hipMemsetAsync(s.counter, 0, sizeof(unsigned long long), st));
  const int64_t want = (count + 255) / 256;
  const uint32_t blocks = (uint32_t)(want < 8192 ? want : 8192);
  if (dtype == NEPTUNE_HIP_F64)
    hipLaunchKernelGGL(neptune_count_mismatch<unsigned long long>, dim3(blocks), dim3(256), 0, st,
                       (const unsigned long long*)a, (const unsigned long long*)b, count, s.counter);
  else
    hipLaunchKernelGGL(neptune_count_mismatch<unsigned int>, dim3(blocks), dim3(256), 0, st,
                       (const unsigned int*)a, (const unsigned int*)b, count, s.counter);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  unsigned long long host = 0;
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(&host, s.counter, sizeof(host), hipMemcpyDeviceToHost, st));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(st));
  return (int64_t)host;
}

double neptune_hip_time_apply_builtin(int body, const neptune_hip_apply_geom_t* g, const void* const* in,
                                      void* out, void* stream, const neptune_hip_launch_cfg_t* cfg, int warmup,
                                      int reps) {
  return time_launches([&](const neptune_hip_launch_cfg_t* c) { return neptune_hip_apply_builtin(body, g, in, out, stream, c); },
                       as_stream(stream), cfg, warmup, reps);
}

double neptune_hip_time_apply_fn(neptune_hip_apply_fn fn, const neptune_hip_apply_geom_t* g, const void* const* in,
                                 void* out, void* stream, const neptune_hip_launch_cfg_t* cfg, int warmup, int reps) {
  if (!fn) return (double)NEPTUNE_HIP_EINVAL;
  return time_launches([&](const neptune_hip_launch_cfg_t* c) { return fn(g, in, out, stream, c); }, as_stream(stream), cfg,
                       warmup, reps);
}

int neptune_hip_autotune_builtin(int body, const neptune_hip_apply_geom_t* g, const void* const* in, void* out,
                                 void* stream, int reps, neptune_hip_launch_cfg_t* best, double* best_ms) {
  if (!g || !in || !out || !best) return NEPTUNE_HIP_EINVAL;
  neptune_hip_launch_cfg_t probe = {NEPTUNE_HIP_KERNEL_AUTO, -1, 0, 0};
  const int planned = neptune_hip_apply_builtin_plan(body, g, in, out, &probe);
  if (planned < 0) return planned;
  return autotune_launches([&](const neptune_hip_launch_cfg_t* c) { return neptune_hip_apply_builtin(body, g, in, out, stream, c); },
                           planned == NEPTUNE_HIP_KERNEL_MARCH, g->rank, march_variant_count(g->rank), as_stream(stream), reps,
                           best, best_ms);
}

int neptune_hip_autotune_fn(neptune_hip_apply_fn fn, int num_variants, const neptune_hip_apply_geom_t* g,
                            const void* const* in, void* out, void* stream, int reps, neptune_hip_launch_cfg_t* best,
                            double* best_ms) {
  if (!fn || !g || !in || !out || !best) return NEPTUNE_HIP_EINVAL;
  if (g->rank < 1 || g->rank > kMaxRank) return NEPTUNE_HIP_EINVAL;
  // whether the automatic launch is a march launch is the module's business; a forced march tile that cannot take
  // the geometry is rejected by the entry itself (negative return) and simply never becomes the best
  const int nv = num_variants < 0 ? 0 : (num_variants < march_variant_count(g->rank) ? num_variants : march_variant_count(g->rank));
  return autotune_launches([&](const neptune_hip_launch_cfg_t* c) { return fn(g, in, out, stream, c); }, nv > 0, g->rank, nv,
                           as_stream(stream), reps, best, best_ms);
}

double neptune_hip_time_copy(void* dst, const void* src, size_t bytes, void* stream, int mode, int warmup,
                             int reps) {
  if (!dst || !src || reps <= 0 || bytes % 16 != 0) return -1.0;
  ensure_init();
  hipStream_t st = as_stream(stream);
  const int64_t n16 = (int64_t)(bytes / 16);
  auto blocks_for = [&](int U) { return (uint32_t)((n16 + 256 * U - 1) / (256 * U)); };
  auto launch = [&] {
    const u32x4* s4 = (const u32x4*)src;
    u32x4* d4 = (u32x4*)dst;
    switch (mode) {
      default:
      case 0:  // grid-stride, 8 workgroups per CU
        hipLaunchKernelGGL(neptune_copy16, dim3(256 * 8), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, n16);
        break;
      case 1: hipLaunchKernelGGL((neptune_copy16_unrolled<4, false, false>), dim3(blocks_for(4)), dim3(256), 0, st, s4, d4, n16); break;
      case 2: hipLaunchKernelGGL((neptune_copy16_unrolled<4, false, true>), dim3(blocks_for(4)), dim3(256), 0, st, s4, d4, n16); break;
      case 3: hipLaunchKernelGGL((neptune_copy16_unrolled<4, true, true>), dim3(blocks_for(4)), dim3(256), 0, st, s4, d4, n16); break;
      case 4: hipLaunchKernelGGL((neptune_copy16_unrolled<8, false, true>), dim3(blocks_for(8)), dim3(256), 0, st, s4, d4, n16); break;
      case 5: hipLaunchKernelGGL((neptune_copy16_unrolled<1, false, true>), dim3(blocks_for(1)), dim3(256), 0, st, s4, d4, n16); break;
      case 6: hipLaunchKernelGGL((neptune_copy16_unrolled<2, false, true>), dim3(blocks_for(2)), dim3(256), 0, st, s4, d4, n16); break;
    }
  };
  for (int i = 0; i < warmup; ++i) launch();
  hipEvent_t e0, e1;
  NEPTUNE_HIP_CHECK(hipEventCreate(&e0));
  NEPTUNE_HIP_CHECK(hipEventCreate(&e1));
  NEPTUNE_HIP_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i) launch();
  NEPTUNE_HIP_CHECK(hipEventRecord(e1, st));
  NEPTUNE_HIP_CHECK(hipEventSynchronize(e1));
  NEPTUNE_HIP_CHECK(hipGetLastError());
  float ms = 0.f;
  NEPTUNE_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  NEPTUNE_HIP_CHECK(hipEventDestroy(e0));
  NEPTUNE_HIP_CHECK(hipEventDestroy(e1));
  return (double)ms / reps;
}
int neptune_hip_copy_mode_count(void) { return 7; }

void* neptune_hip_event_create(void) {
  ensure_init();
  hipEvent_t e;
  NEPTUNE_HIP_CHECK(hipEventCreate(&e));
  return (void*)e;
}
void neptune_hip_event_destroy(void* ev) {
  if (ev) NEPTUNE_HIP_CHECK(hipEventDestroy((hipEvent_t)ev));
}
void neptune_hip_event_record(void* ev, void* stream) {
  NEPTUNE_HIP_CHECK(hipEventRecord((hipEvent_t)ev, as_stream(stream)));
}
void neptune_hip_event_sync(void* ev) { NEPTUNE_HIP_CHECK(hipEventSynchronize((hipEvent_t)ev)); }
double neptune_hip_event_elapsed_ms(void* start, void* stop) {
  float ms = 0.f;
  NEPTUNE_HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop));
  return (double)ms;
}
void neptune_hip_stream_wait_event(void* stream, void* ev) {
  NEPTUNE_HIP_CHECK(hipStreamWaitEvent(as_stream(stream), (hipEvent_t)ev, 0));
}

}  // extern "C"
