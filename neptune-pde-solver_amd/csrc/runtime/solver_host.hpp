// solver_host.hpp -- what the host code of step_loop.hip and multigrid.hip shares, each rule once: the small helpers, the
// element type of an entry, the capture query, the stream scope (ONE bridge stream for the whole library), the read-back of
// device scalars, the outer operator of a Krylov solve and the bookkeeping of a solver's out-parameters.  Host code only,
// internal: nothing in here is exported from the shared library.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"   // NEPTUNE_HIP_CHECK

#pragma GCC visibility push(hidden)
namespace neptune_hip {

// step_loop.hip: destroys the cached graphs of the step loops and frees the solvers' device blocks, for neptune_hip_finalize
void step_loop_destroy_graphs();
// neptune_hip_rt.hip: brings the runtime up (on device 0) unless it is up already
void ensure_init();

// ---------------------------------------------------------------- small helpers
// the cfg to launch with: nullptr unless the caller set anything
inline const neptune_hip_launch_cfg_t* set_cfg(const neptune_hip_launch_cfg_t* cfg) {
  return (cfg && (cfg->kernel || cfg->variant >= 0 || cfg->chunk || cfg->flags)) ? cfg : nullptr;
}

inline bool known_dtype(int dtype) { return dtype == NEPTUNE_HIP_F64 || dtype == NEPTUNE_HIP_F32; }
inline size_t elem_size(int dtype) { return dtype == NEPTUNE_HIP_F64 ? 8 : 4; }

// a launch's error, or what a unit (an iteration, a cycle) answers for it: after the unit's first launch the fields have
// moved, so a refusal from there is an error
inline int late(int rc) { return rc == NEPTUNE_HIP_EUNSUPPORTED ? NEPTUNE_HIP_EINVAL : rc; }

// whether the launch region is the whole box (an apply stores nothing outside its launch region)
inline bool region_is_whole(const neptune_hip_apply_geom_t* g) {
  bool whole = true;
  for (int d = 0; d < g->rank; ++d) whole = whole && g->region_lb[d] <= 0 && g->region_ub[d] >= g->out_ub[d] - g->out_lb[d];
  return whole;
}

// ---------------------------------------------------------------- entry type
// the element type of a built-in body; the caller has checked 0 <= body < NEPTUNE_HIP_BODY_COUNT
inline int body_dtype(int body) { return body == NEPTUNE_HIP_BODY_LAP3D27_F32 ? NEPTUNE_HIP_F32 : NEPTUNE_HIP_F64; }
// The element type of an entry: a lowered `fn` brings its own dtype_of_fn, a built-in body (fn = nullptr) has body_dtype.
// -> false: a body out of range or a type that is neither f64 nor f32.  No HIP call.
inline bool entry_dtype(neptune_hip_apply_fn fn, int body, int dtype_of_fn, int* dtype) {
  if (!fn && (body < 0 || body >= NEPTUNE_HIP_BODY_COUNT)) return false;
  *dtype = fn ? dtype_of_fn : body_dtype(body);
  return known_dtype(*dtype);
}

// ---------------------------------------------------------------- capture query
// whether `stream` is being captured into a graph.  A null stream (the legacy default stream cannot be captured) answers
// false without any HIP call; a failed query clears the error and answers false.
inline bool stream_capturing(void* stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(reinterpret_cast<hipStream_t>(stream), &cs) != hipSuccess) {
    (void)hipGetLastError();
    cs = hipStreamCaptureStatusNone;
  }
  return cs != hipStreamCaptureStatusNone;
}

// ---------------------------------------------------------------- stream scope
// the one bridge of the library: stands in for the legacy default stream, which cannot be captured.  Created at first use,
// never destroyed.
inline hipStream_t g_bridge_stream = nullptr;
inline hipEvent_t g_bridge_ev[2] = {nullptr, nullptr};

// The stream a loop or a solve runs on, and whether the caller is capturing it.  The legacy default stream cannot be
// captured: the work then runs on the bridge stream, ordered after everything already queued on the default stream, and the
// destructor orders the default stream after the work -- on every exit path.
struct StreamScope {
  hipStream_t stream;
  bool capturing;
  const bool bridged;
  explicit StreamScope(hipStream_t user) : stream(user), bridged(!user) {
    if (bridged) {
      if (!g_bridge_stream) {
        NEPTUNE_HIP_CHECK(hipStreamCreateWithFlags(&g_bridge_stream, hipStreamNonBlocking));
        NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_bridge_ev[0], hipEventDisableTiming));
        NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_bridge_ev[1], hipEventDisableTiming));
      }
      NEPTUNE_HIP_CHECK(hipEventRecord(g_bridge_ev[0], nullptr));
      NEPTUNE_HIP_CHECK(hipStreamWaitEvent(g_bridge_stream, g_bridge_ev[0], 0));
      stream = g_bridge_stream;
    }
    capturing = stream_capturing((void*)stream);
  }
  ~StreamScope() {
    if (bridged) {
      NEPTUNE_HIP_CHECK(hipEventRecord(g_bridge_ev[1], g_bridge_stream));
      NEPTUNE_HIP_CHECK(hipStreamWaitEvent(nullptr, g_bridge_ev[1], 0));
    }
  }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};

// ---------------------------------------------------------------- scalar read-back
// `count` (1 or 2) consecutive device scalars, after everything queued on the stream: one synchronise
template <class T>
void read_scalars(hipStream_t stream, const T* dev, int count, double* host) {
  T h[2] = {0, 0};
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(h, dev, (size_t)count * sizeof(T), hipMemcpyDeviceToHost, stream));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
  for (int i = 0; i < count; ++i) host[i] = (double)h[i];
}
// two scalars at separate addresses: still one synchronise
template <class T>
void read_scalars(hipStream_t stream, const T* dev0, double* host0, const T* dev1, double* host1) {
  T h[2] = {0, 0};
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h[0], dev0, sizeof(T), hipMemcpyDeviceToHost, stream));
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h[1], dev1, sizeof(T), hipMemcpyDeviceToHost, stream));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
  *host0 = (double)h[0];
  *host1 = (double)h[1];
}
// the consecutive form for a type known at run time
inline void read_scalars(int dtype, hipStream_t stream, const void* dev, int count, double* host) {
  if (dtype == NEPTUNE_HIP_F64) read_scalars(stream, static_cast<const double*>(dev), count, host);
  else read_scalars(stream, static_cast<const float*>(dev), count, host);
}

// ---------------------------------------------------------------- outer operator
// The operator A of a Krylov solve: a lowered entry `fn` (with its dot-monitored form fn_dot, or nullptr) or a built-in
// body, the geometry, the fixed inputs behind input 0, the cfg to launch with (set_cfg's) and the stream.  Only the launches:
// what a solver does about a refusal of the dot-monitored entry is the solver's own.
struct OuterOperator {
  neptune_hip_apply_fn fn;
  neptune_hip_apply_dot_fn fn_dot;
  int body;
  const neptune_hip_apply_geom_t* g;
  const void* const* in_rest;
  const neptune_hip_launch_cfg_t* cfg;
  hipStream_t stream;

  // whether there is a dot-monitored entry to ask at all
  bool has_dot() const { return fn ? fn_dot != nullptr : true; }
  void inputs(const void** ins, const void* in0) const {
    ins[0] = in0;
    for (int i = 1; i < g->num_inputs; ++i) ins[i] = in_rest[i - 1];
  }
  // out = A(in0), a plain launch
  int apply(const void* in0, void* out) const {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    inputs(ins, in0);
    return fn ? fn(g, ins, out, (void*)stream, cfg) : neptune_hip_apply_builtin(body, g, ins, out, (void*)stream, cfg);
  }
  // out = A(in0) and *dot_dev = out . in0 out of one dot-monitored launch; NEPTUNE_HIP_EUNSUPPORTED: nothing was launched
  int apply_dot(const void* in0, void* out, void* dot_dev) const {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    inputs(ins, in0);
    return fn ? fn_dot(g, ins, out, dot_dev, (void*)stream, cfg) : neptune_hip_apply_builtin_dot(body, g, ins, out, dot_dev, (void*)stream, cfg);
  }
};

// ---------------------------------------------------------------- result bookkeeping
// a solver entry's out-parameters (each optional) before anything is checked
inline void reset_solver_outputs(int64_t* iters_done, double* rr0, double* rr_last) {
  if (iters_done) *iters_done = 0;
  if (rr0) *rr0 = 0.0;
  if (rr_last) *rr_last = 0.0;
}
// rr_0 is known: -> whether there is nothing to iterate
inline bool done_after_setup(double rr, double tol2, int64_t max_iters, double* rr0, double* rr_last) {
  if (rr0) *rr0 = rr;
  if (rr_last) *rr_last = rr;
  return rr <= tol2 || max_iters == 0;
}

}  // namespace neptune_hip
#pragma GCC visibility pop
