// multigrid.hip -- include/neptune_hip.h: geometric multigrid V-cycles over a hierarchy of applies.
// neptune_hip_mg_smooth / _restrict / _prolong_add launch the three kernels of multigrid_kernels.hpp alone;
// neptune_hip_mg_solve is the cycle driver: the levels' operators through the public C API, the kernels in between, r . r
// through neptune_hip_update_norm, and its own small capture / replay of ONE cycle (a linear graph on the call's stream,
// captured once per call, destroyed when the call returns).  Its own translation unit (builds in seconds, linked into
// libneptune_hip.so): host code plus the three kernels' instantiations.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"   // NEPTUNE_HIP_CHECK, geom_validate, buffers_overlap (no apply kernel is instantiated here)
#include "../kernels/multigrid_kernels.hpp"

using namespace neptune_hip;

namespace {

constexpr int kMaxLevels = 16;

// what neptune_hip_rt.hip's ensure_init does (device 0 unless the runtime is up already), through the public API
void ensure_init() { (void)neptune_hip_cu_count(); }

bool known_dtype(int dtype) { return dtype == NEPTUNE_HIP_F64 || dtype == NEPTUNE_HIP_F32; }
size_t elem_size(int dtype) { return dtype == NEPTUNE_HIP_F64 ? 8 : 4; }

// A level's box and Omega = apply.bounds x launch region on the kernels' three axes (the field's dimensions right-aligned);
// -> false for a malformed geometry, an input 0 in another box than the result's, or an empty Omega
bool level_box(const neptune_hip_apply_geom_t* g, MgBox& B) {
  if (!g || geom_validate(g) != NEPTUNE_HIP_OK) return false;
  for (int a = 0; a < 3; ++a) {
    B.n[a] = 1;
    B.lo[a] = 0;
    B.m[a] = 1;
  }
  for (int d = 0; d < g->rank; ++d) {
    if (g->in_lb[0][d] != g->out_lb[d] || g->in_ub[0][d] != g->out_ub[d]) return false;
    const int a = d + 3 - g->rank;
    const int64_t n = g->out_ub[d] - g->out_lb[d];
    const int64_t lo = std::max<int64_t>(std::max(g->lb[d] - g->out_lb[d], g->region_lb[d]), 0);
    const int64_t hi = std::min(std::min(g->ub[d] - g->out_lb[d], g->region_ub[d]), n);
    if (hi <= lo) return false;
    B.n[a] = n;
    B.lo[a] = lo;
    B.m[a] = hi - lo;
  }
  return true;
}
// m_fine = 2 m_coarse + 1 on every axis that carries a dimension
bool sizes_nest(const MgBox& F, const MgBox& Cb, int rank) {
  for (int a = 3 - rank; a < 3; ++a)
    if (F.m[a] != 2 * Cb.m[a] + 1) return false;
  return true;
}
size_t box_bytes(const MgBox& B, size_t elem) { return (size_t)(B.n[0] * B.n[1] * B.n[2]) * elem; }

struct RowGrid {
  int64_t nchunk;
  dim3 grid;
};
// one workgroup per 256-cell chunk of a row of B's Omega
RowGrid row_grid(const MgBox& B) {
  RowGrid r;
  r.nchunk = (B.m[2] + 255) / 256;
  r.grid = grid_for_blocks(B.m[0] * B.m[1] * r.nchunk);
  return r;
}

int launched() { return hipGetLastError() == hipSuccess ? NEPTUNE_HIP_OK : NEPTUNE_HIP_EUNSUPPORTED; }

template <class T>
int smooth_launch(const MgBox& B, const void* q, const void* b, const void* minv, void* x, hipStream_t stream) {
  const RowGrid r = row_grid(B);
  hipLaunchKernelGGL(neptune_mg_smooth<T>, r.grid, dim3(256), 0, stream, B, r.nchunk, static_cast<const T*>(q), static_cast<const T*>(b),
                     static_cast<const T*>(minv), static_cast<T*>(x));
  return launched();
}
template <class T, int RANK>
int restrict_launch(const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c, void* x_c,
                    hipStream_t stream) {
  const RowGrid r = row_grid(Cb);
  hipLaunchKernelGGL((neptune_mg_restrict<T, RANK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(b_f),
                     static_cast<const T*>(q_f), (T)rscale, static_cast<T*>(b_c), static_cast<T*>(x_c));
  return launched();
}
template <class T, int RANK>
int prolong_launch(const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t stream) {
  const RowGrid r = row_grid(F);
  hipLaunchKernelGGL((neptune_mg_prolong_add<T, RANK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(x_c),
                     static_cast<T*>(x_f));
  return launched();
}
// the dispatch on element type and rank, stated once
template <class F64, class F32>
int by_type(int dtype, F64&& f64, F32&& f32) { return dtype == NEPTUNE_HIP_F64 ? f64() : f32(); }
int do_smooth(int dtype, const MgBox& B, const void* q, const void* b, const void* minv, void* x, hipStream_t s) {
  return by_type(dtype, [&] { return smooth_launch<double>(B, q, b, minv, x, s); }, [&] { return smooth_launch<float>(B, q, b, minv, x, s); });
}
template <class T>
int restrict_ranked(int rank, const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c, void* x_c,
                    hipStream_t s) {
  if (rank == 3) return restrict_launch<T, 3>(F, Cb, b_f, q_f, rscale, b_c, x_c, s);
  if (rank == 2) return restrict_launch<T, 2>(F, Cb, b_f, q_f, rscale, b_c, x_c, s);
  return restrict_launch<T, 1>(F, Cb, b_f, q_f, rscale, b_c, x_c, s);
}
int do_restrict(int dtype, int rank, const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c,
                void* x_c, hipStream_t s) {
  return by_type(dtype, [&] { return restrict_ranked<double>(rank, F, Cb, b_f, q_f, rscale, b_c, x_c, s); },
                 [&] { return restrict_ranked<float>(rank, F, Cb, b_f, q_f, rscale, b_c, x_c, s); });
}
template <class T>
int prolong_ranked(int rank, const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t s) {
  if (rank == 3) return prolong_launch<T, 3>(F, Cb, x_c, x_f, s);
  if (rank == 2) return prolong_launch<T, 2>(F, Cb, x_c, x_f, s);
  return prolong_launch<T, 1>(F, Cb, x_c, x_f, s);
}
int do_prolong(int dtype, int rank, const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t s) {
  return by_type(dtype, [&] { return prolong_ranked<double>(rank, F, Cb, x_c, x_f, s); },
                 [&] { return prolong_ranked<float>(rank, F, Cb, x_c, x_f, s); });
}

bool stream_capturing(void* stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(reinterpret_cast<hipStream_t>(stream), &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  return cs != hipStreamCaptureStatusNone;
}

// The stream a solve runs on.  The legacy default stream cannot be captured: the solve then runs on an internal stream
// ordered after everything already queued on the default stream, and the destructor orders the default stream after it.
hipStream_t g_mg_stream = nullptr;
hipEvent_t g_mg_ev[2] = {nullptr, nullptr};
struct SolveStream {
  hipStream_t stream;
  const bool bridged;
  explicit SolveStream(hipStream_t user) : stream(user), bridged(!user) {
    if (!bridged) return;
    if (!g_mg_stream) {
      NEPTUNE_HIP_CHECK(hipStreamCreateWithFlags(&g_mg_stream, hipStreamNonBlocking));
      NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_mg_ev[0], hipEventDisableTiming));
      NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_mg_ev[1], hipEventDisableTiming));
    }
    NEPTUNE_HIP_CHECK(hipEventRecord(g_mg_ev[0], nullptr));
    NEPTUNE_HIP_CHECK(hipStreamWaitEvent(g_mg_stream, g_mg_ev[0], 0));
    stream = g_mg_stream;
  }
  ~SolveStream() {
    if (!bridged) return;
    NEPTUNE_HIP_CHECK(hipEventRecord(g_mg_ev[1], g_mg_stream));
    NEPTUNE_HIP_CHECK(hipStreamWaitEvent(nullptr, g_mg_ev[1], 0));
  }
  SolveStream(const SolveStream&) = delete;
  SolveStream& operator=(const SolveStream&) = delete;
};

int64_t g_mg_counts[3] = {0, 0, 0};   // plain cycles, graph cycles, checks of the last solve

// one solve, its arguments checked
struct Solve {
  const neptune_hip_mg_level_t* levels;
  int n_levels, dtype, rank, pre, post, coarse_sweeps;
  MgBox box[kMaxLevels];
  const neptune_hip_launch_cfg_t* cfg;   // level 0's, nullptr unless the caller set anything
  hipStream_t stream;

  // q_l = A_l(x_l), a plain launch
  int apply(int l) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    ins[0] = L.x;
    for (int i = 1; i < L.g.num_inputs; ++i) ins[i] = L.in_rest[i - 1];
    const neptune_hip_launch_cfg_t* c = l == 0 ? cfg : nullptr;
    return L.fn ? L.fn(&L.g, ins, L.q, (void*)stream, c) : neptune_hip_apply_builtin(L.body, &L.g, ins, L.q, (void*)stream, c);
  }
  int sweeps(int l, int count) const {
    const neptune_hip_mg_level_t& L = levels[l];
    for (int s = 0; s < count; ++s) {
      int rc = apply(l);
      if (rc != NEPTUNE_HIP_OK) return rc;
      rc = do_smooth(dtype, box[l], L.q, L.b, L.minv, L.x, stream);
      if (rc != NEPTUNE_HIP_OK) return rc;
    }
    return NEPTUNE_HIP_OK;
  }
  int cycle(int l) const {
    if (l == n_levels - 1) return sweeps(l, coarse_sweeps);
    const neptune_hip_mg_level_t& F = levels[l];
    const neptune_hip_mg_level_t& Cl = levels[l + 1];
    int rc = sweeps(l, pre);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = apply(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = do_restrict(dtype, rank, box[l], box[l + 1], F.b, F.q, F.rscale, Cl.b, Cl.x, stream);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = cycle(l + 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = do_prolong(dtype, rank, box[l], box[l + 1], Cl.x, F.x, stream);
    if (rc != NEPTUNE_HIP_OK) return rc;
    return sweeps(l, post);
  }
  // rr = sum over Omega_0 of (b - A(x))^2 into *rr_dev, then read back: one stream synchronise, one scalar
  int residual(void* rr_dev, double* rr) const {
    int rc = apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = neptune_hip_update_norm(dtype, &levels[0].g, levels[0].b, levels[0].q, rr_dev, (void*)stream);
    if (rc != NEPTUNE_HIP_OK) return rc;
    double h64 = 0.0;
    float h32 = 0.0f;
    void* h = dtype == NEPTUNE_HIP_F64 ? (void*)&h64 : (void*)&h32;
    NEPTUNE_HIP_CHECK(hipMemcpyAsync(h, rr_dev, elem_size(dtype), hipMemcpyDeviceToHost, stream));
    NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
    *rr = dtype == NEPTUNE_HIP_F64 ? h64 : (double)h32;
    return NEPTUNE_HIP_OK;
  }
  // One cycle as a graph: captured on the stream (nothing runs), instantiated; nullptr when any launch refused under
  // capture or the runtime would not have the graph -- the caller goes on with plain launches.
  hipGraphExec_t capture(hipGraph_t* graph_out) const {
    *graph_out = nullptr;
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const int rc = cycle(0);
    hipGraph_t graph = nullptr;
    if (hipStreamEndCapture(stream, &graph) != hipSuccess) { (void)hipGetLastError(); graph = nullptr; }
    if (rc != NEPTUNE_HIP_OK || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      return nullptr;
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipGraphDestroy(graph);
      return nullptr;
    }
    *graph_out = graph;
    return exec;
  }
};

// a late refusal: after the first launch of a cycle the fields have moved
int late(int rc) { return rc == NEPTUNE_HIP_EUNSUPPORTED ? NEPTUNE_HIP_EINVAL : rc; }

bool graph_path_enabled() {
  const char* e = getenv("NEPTUNE_HIP_MG_GRAPH");
  return !(e && strcmp(e, "0") == 0);
}

}  // namespace

extern "C" {

int neptune_hip_mg_smooth(int dtype, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                          void* stream) {
  if (!g || !q || !b || !minv || !x || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, elem_size(dtype));
  if (buffers_overlap(x, bytes, q, bytes) || buffers_overlap(x, bytes, b, bytes) || buffers_overlap(x, bytes, minv, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_smooth(dtype, B, q, b, minv, x, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_restrict(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                            const void* b_fine, const void* q_fine, double rscale, void* b_coarse, void* x_coarse, void* stream) {
  if (!g_fine || !g_coarse || !b_fine || !q_fine || !b_coarse || !x_coarse || !known_dtype(dtype) || !isfinite(rscale)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  if (g_fine->rank != g_coarse->rank || !sizes_nest(F, Cb, g_fine->rank)) return NEPTUNE_HIP_EINVAL;
  const size_t fb = box_bytes(F, elem_size(dtype)), cb = box_bytes(Cb, elem_size(dtype));
  if (buffers_overlap(b_coarse, cb, x_coarse, cb)) return NEPTUNE_HIP_EINVAL;
  for (const void* w : {(const void*)b_coarse, (const void*)x_coarse})
    if (buffers_overlap(w, cb, b_fine, fb) || buffers_overlap(w, cb, q_fine, fb)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_restrict(dtype, g_fine->rank, F, Cb, b_fine, q_fine, rscale, b_coarse, x_coarse, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_prolong_add(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                               const void* x_coarse, void* x_fine, void* stream) {
  if (!g_fine || !g_coarse || !x_coarse || !x_fine || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  if (g_fine->rank != g_coarse->rank || !sizes_nest(F, Cb, g_fine->rank)) return NEPTUNE_HIP_EINVAL;
  if (buffers_overlap(x_fine, box_bytes(F, elem_size(dtype)), x_coarse, box_bytes(Cb, elem_size(dtype)))) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_prolong(dtype, g_fine->rank, F, Cb, x_coarse, x_fine, reinterpret_cast<hipStream_t>(stream));
}

void neptune_hip_mg_counts(int64_t* plain_cycles, int64_t* graph_cycles, int64_t* checks) {
  if (plain_cycles) *plain_cycles = g_mg_counts[0];
  if (graph_cycles) *graph_cycles = g_mg_counts[1];
  if (checks) *checks = g_mg_counts[2];
}

int neptune_hip_mg_solve(const neptune_hip_mg_level_t* levels, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                         int64_t max_cycles, int64_t check_every, double tol2, double* rr_checks, void* stream,
                         const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done, double* rr0, double* rr_last) {
  g_mg_counts[0] = g_mg_counts[1] = g_mg_counts[2] = 0;
  if (cycles_done) *cycles_done = 0;
  if (rr0) *rr0 = 0.0;
  if (rr_last) *rr_last = 0.0;
  // ---- the refusals, before anything touches the device
  if (!levels || n_levels < 1 || n_levels > kMaxLevels || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  if (pre < 0 || post < 0 || coarse_sweeps < 0 || check_every < 1 || max_cycles < 0) return NEPTUNE_HIP_EINVAL;
  Solve S;
  S.levels = levels;
  S.n_levels = n_levels;
  S.dtype = dtype;
  S.pre = pre;
  S.post = post;
  S.coarse_sweeps = coarse_sweeps;
  S.cfg = (cfg && (cfg->kernel || cfg->variant >= 0 || cfg->chunk || cfg->flags)) ? cfg : nullptr;
  S.rank = levels[0].g.rank;
  const size_t elem = elem_size(dtype);
  for (int l = 0; l < n_levels; ++l) {
    const neptune_hip_mg_level_t& L = levels[l];
    if (!L.x || !L.b || !L.q || !L.minv) return NEPTUNE_HIP_EINVAL;
    if (!level_box(&L.g, S.box[l]) || L.g.rank != S.rank) return NEPTUNE_HIP_EINVAL;
    if (!L.fn) {
      if (L.body < 0 || L.body >= NEPTUNE_HIP_BODY_COUNT) return NEPTUNE_HIP_EINVAL;
      if ((L.body == NEPTUNE_HIP_BODY_LAP3D27_F32 ? NEPTUNE_HIP_F32 : NEPTUNE_HIP_F64) != dtype) return NEPTUNE_HIP_EINVAL;
    }
    if (L.g.num_inputs > 1 && !L.in_rest) return NEPTUNE_HIP_EINVAL;
    for (int i = 1; i < L.g.num_inputs; ++i)
      if (!L.in_rest[i - 1]) return NEPTUNE_HIP_EINVAL;
    if (l + 1 < n_levels && !isfinite(L.rscale)) return NEPTUNE_HIP_EINVAL;
    if (l > 0 && !sizes_nest(S.box[l - 1], S.box[l], S.rank)) return NEPTUNE_HIP_EINVAL;
    const void* mine[4] = {L.x, L.b, L.q, L.minv};
    const size_t bytes = box_bytes(S.box[l], elem);
    for (int a = 0; a < 4; ++a) {
      if ((uintptr_t)mine[a] % elem != 0) return NEPTUNE_HIP_EINVAL;
      for (int o = 0; o < a; ++o)
        if (buffers_overlap(mine[a], bytes, mine[o], bytes)) return NEPTUNE_HIP_EINVAL;
      if (l > 0) {
        const neptune_hip_mg_level_t& P = levels[l - 1];
        const void* finer[4] = {P.x, P.b, P.q, P.minv};
        const size_t finer_bytes = box_bytes(S.box[l - 1], elem);
        for (int o = 0; o < 4; ++o)
          if (buffers_overlap(mine[a], bytes, finer[o], finer_bytes)) return NEPTUNE_HIP_EINVAL;
      }
    }
  }
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  SolveStream sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  struct Scalar {   // one device T for r . r, this call's
    void* p = nullptr;
    Scalar() { NEPTUNE_HIP_CHECK(hipMalloc(&p, 8)); }
    ~Scalar() { (void)hipFree(p); }
  } rr_dev;
  struct Graph {    // this call's graph of one cycle
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~Graph() {
      if (exec) (void)hipGraphExecDestroy(exec);
      if (graph) (void)hipGraphDestroy(graph);
    }
  } G;

  for (int l = 1; l < n_levels; ++l) NEPTUNE_HIP_CHECK(hipMemsetAsync(levels[l].x, 0, box_bytes(S.box[l], elem), S.stream));
  double rr = 0.0;
  int rc = S.residual(rr_dev.p, &rr);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (rr0) *rr0 = rr;
  if (rr_last) *rr_last = rr;
  if (rr <= tol2) return NEPTUNE_HIP_OK;

  const bool graphs = graph_path_enabled();
  bool capture_tried = false;
  int64_t done = 0;
  while (done < max_cycles) {
    const int64_t block = check_every < max_cycles - done ? check_every : max_cycles - done;
    for (int64_t c = 0; c < block; ++c, ++done) {
      // the first cycle plain: it validates the request and lets first-use tuning run outside capture; then, when at least
      // two more cycles may follow, ONE capture
      if (done > 0 && graphs && !capture_tried && max_cycles - done >= 2) {
        capture_tried = true;
        G.exec = S.capture(&G.graph);
      }
      if (done > 0 && G.exec) {
        NEPTUNE_HIP_CHECK(hipGraphLaunch(G.exec, S.stream));
        ++g_mg_counts[1];
      } else {
        rc = S.cycle(0);
        if (rc != NEPTUNE_HIP_OK) return late(rc);
        ++g_mg_counts[0];
      }
      if (cycles_done) *cycles_done = done + 1;
    }
    rc = S.residual(rr_dev.p, &rr);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    if (rr_checks) rr_checks[g_mg_counts[2]] = rr;
    ++g_mg_counts[2];
    if (rr_last) *rr_last = rr;
    if (rr <= tol2) break;   // false for a NaN: such a solve runs to max_cycles
  }
  return NEPTUNE_HIP_OK;
}

}  // extern "C"
