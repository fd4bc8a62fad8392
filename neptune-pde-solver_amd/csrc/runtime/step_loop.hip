// step_loop.hip -- include/neptune_hip.h: the hipGraph step loops.  One replay engine (graph cache, replay, grouping choice,
// on the stream scope of solver_host.hpp) that knows nothing about ping-pong or leapfrog, and the three loops built on it:
// neptune_hip_step_loop_chain (one-level schemes, two fields), neptune_hip_step_loop_leapfrog (two-level schemes, three or
// four fields) and neptune_hip_step_loop_system (a group of sibling applies: two SETS of fields); and the Krylov solvers
// neptune_hip_cg_solve / neptune_hip_pcg_solve / neptune_hip_bicgstab_solve, whose iteration the same engine replays: ONE
// host schedule (SolverFrame: the key, blocks of iterations, the counters), and per solver its set-up and its iteration.
// What multigrid.hip needs as well -- the stream scope, the capture query, the operator's launches, the read-back, the
// out-parameters -- is solver_host.hpp's.  Its own translation unit (builds in seconds, linked into libneptune_hip.so): host
// code that launches applies through the public C API, plus the solvers' few vector kernels (krylov_kernels.hpp).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"   // NEPTUNE_HIP_CHECK, tune_mode (no apply kernel is instantiated here)
#include "../kernels/krylov_kernels.hpp"
#include "solver_host.hpp"

using namespace neptune_hip;

namespace {

// ---------------------------------------------------------------- what a loop is: the key of both caches
using group_fn = void (*)();   // an entry of a larger grouping, untyped: the caches only compare it
struct LoopKey {
  neptune_hip_apply_fn fn;     // the single-step entry (launch kind 1), or nullptr: built-in body `body`
  int body;
  // the optional entries of launch kinds 2 and 3, nullptr = none: <tag>__geom2 / __geom3 in the one-level loop,
  // <tag>__geomL2 / nothing in the leapfrog loop (two loops cannot meet in a cache: their entry types differ)
  group_fn more[2];
  neptune_hip_apply_geom_t g;
  void* fields[4];             // the rotating fields, nullptr beyond the loop's own two, three or four
  // the system loop: fields[] is set A of its n_out unknowns, fields_b[] set B, through[m] the union input member m advances;
  // n_out = 0 and the rest zero in the other loops
  void* fields_b[4];
  void* fields_c[4];           // the BiCGStab solver's further vectors (its iteration touches more than eight buffers); zero elsewhere
  int through[4];
  int n_out;
  const void* in[NEPTUNE_HIP_MAX_INPUTS];   // the inputs that are no state (centre-only inputs: the same field at every stage)
  neptune_hip_launch_cfg_t cfg;
  hipStream_t stream;
  int kind, state;             // (graph cache only) what one node of the graph is, and the rotation state at graph start
};
// the part of a key that is common to every loop; padding too: keys are compared with memcmp
void init_key(LoopKey& k, neptune_hip_apply_fn fn, int body, const neptune_hip_apply_geom_t* g, const neptune_hip_launch_cfg_t* cfg,
              hipStream_t stream) {
  memset(&k, 0, sizeof(k));
  k.fn = fn;
  k.body = body;
  k.g = *g;
  if (cfg) k.cfg = *cfg; else k.cfg.variant = -1;
  k.stream = stream;
}
const neptune_hip_launch_cfg_t* loop_cfg(const LoopKey& k) { return set_cfg(&k.cfg); }
// the inputs of one launch: the state in fields[cur], a two-level scheme's previous state in fields[prev] (-1: none), the rest
// riding along unchanged
void loop_inputs(const LoopKey& k, const void** ins, int cur, int prev) {
  for (int i = 0; i < k.g.num_inputs; ++i) ins[i] = k.in[i];
  ins[0] = k.fields[cur];
  if (prev >= 0) ins[1] = k.fields[prev];
}

// ---------------------------------------------------------------- graph cache
struct LoopGraph {
  LoopKey key;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint64_t stamp = 0;
};
constexpr int kLoopGraphs = 8;
LoopGraph g_loops[kLoopGraphs];
uint64_t g_loop_clock = 0;
std::mutex g_loop_mu;

void destroy_graph(LoopGraph& e) {
  if (!e.exec) return;
  (void)hipGraphExecDestroy(e.exec);
  (void)hipGraphDestroy(e.graph);
  e.exec = nullptr;
  e.graph = nullptr;
}

// The cached graph of `gkey`, captured on `stream` at first use: record() issues the launches of one period (a sequence
// that leaves the state where it found it, so the graph can be replayed any number of times) and returns their first
// error.  Graphs are cached by geometry, pointers, configuration and kind; the least recently used one makes room.
// nullptr and *rc on failure.  The caller holds g_loop_mu.
template <class R>
LoopGraph* loop_graph(const LoopKey& gkey, hipStream_t stream, R&& record, int* rc) {
  LoopGraph* slot = nullptr;
  for (auto& e : g_loops)
    if (e.exec && memcmp(&e.key, &gkey, sizeof(gkey)) == 0) slot = &e;
  if (!slot) {
    slot = &g_loops[0];
    for (auto& e : g_loops)
      if (e.stamp < slot->stamp) slot = &e;  // least recently used (empty slots have stamp 0)
    destroy_graph(*slot);
    NEPTUNE_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
    const int r = record();
    hipGraph_t graph = nullptr;
    NEPTUNE_HIP_CHECK(hipStreamEndCapture(stream, &graph));
    if (r != NEPTUNE_HIP_OK || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      *rc = r != NEPTUNE_HIP_OK ? r : NEPTUNE_HIP_EINVAL;
      return nullptr;
    }
    NEPTUNE_HIP_CHECK(hipGraphInstantiate(&slot->exec, graph, nullptr, nullptr, 0));
    slot->graph = graph;
    memcpy(&slot->key, &gkey, sizeof(gkey));
  }
  slot->stamp = ++g_loop_clock;
  return slot;
}

// ---------------------------------------------------------------- replay
// which of the one-level loop's two fields holds the state
int state_code(int from) { return from; }
// which of the leapfrog loop's (up to) four fields plays which part: cur = u(n), prev = u(n-1), f1 / f2 = the free buffers
struct LeapState { int cur, prev, f1, f2; };
int state_code(const LeapState& s) { return s.cur | s.prev << 2 | s.f1 << 4 | (s.f2 & 3) << 6; }

// `count` launches of one kind from state `s`; launch(kind, s) issues one and, when it succeeds, rotates `s`.  The first
// launch is a plain one: it validates the request and warms the launcher's one-time queries outside of stream capture, and
// its code comes back untouched -- NEPTUNE_HIP_EUNSUPPORTED from the FIRST launch means that nothing has run, and the caller
// may fall back to another grouping.  Then whole graphs of `per_graph` launches, captured once and replayed from the cache, so
// that small fields are not bound by launch overhead; per_graph is a multiple of the rotation's period, so a graph leaves
// the state where it found it.  Not inside a caller's capture: a capturing stream cannot begin another one.  Then the rest
// plain.  After the first launch the state has moved, so a late NEPTUNE_HIP_EUNSUPPORTED is an error: NEPTUNE_HIP_EINVAL.
// *graph_launches (optional): how many hipGraphLaunch calls carried launches of this run.
template <class State, class Launch>
int replay(LoopKey& key, const StreamScope& sc, int kind, int64_t count, State& s, int per_graph, Launch&& launch,
           int64_t* graph_launches = nullptr) {
  if (count <= 0) return NEPTUNE_HIP_OK;
  int rc = launch(kind, s);
  if (rc != NEPTUNE_HIP_OK) return rc;
  int64_t done = 1;
  if (!sc.capturing && count - done >= per_graph) {
    key.kind = kind;
    key.state = state_code(s);
    std::lock_guard<std::mutex> lk(g_loop_mu);
    LoopGraph* slot = loop_graph(key, sc.stream, [&] {
      State t = s;
      int r = NEPTUNE_HIP_OK;
      for (int i = 0; i < per_graph && r == NEPTUNE_HIP_OK; ++i) r = launch(kind, t);
      return r;
    }, &rc);
    if (!slot) return rc == NEPTUNE_HIP_EUNSUPPORTED ? NEPTUNE_HIP_EINVAL : rc;
    for (; count - done >= per_graph; done += per_graph) {
      NEPTUNE_HIP_CHECK(hipGraphLaunch(slot->exec, sc.stream));
      if (graph_launches) ++*graph_launches;
    }
  }
  for (; done < count; ++done) {
    rc = launch(kind, s);
    if (rc != NEPTUNE_HIP_OK) return rc == NEPTUNE_HIP_EUNSUPPORTED ? NEPTUNE_HIP_EINVAL : rc;
  }
  return NEPTUNE_HIP_OK;
}

// ---------------------------------------------------------------- grouping choice
// Several steps per launch pay where a step is bound by HBM: a field that stays in the 256 MiB memory-side cache between
// steps gains nothing from saved passes and loses to the chain kernels' longer dependent march (measured,
// profiles/r02_twostep.txt: 128^3 and 1024^2 fp64 are faster one apply per launch, 256^3 and 2048^2 are faster chained: the
// line is 4e6 cells).  NEPTUNE_HIP_NO_PAIRS=1 keeps one step per launch.  Both are read on every call.
bool grouping_allowed(const neptune_hip_apply_geom_t* g) {
  int64_t cells = 1;
  for (int d = 0; d < g->rank; ++d) cells *= g->ub[d] > g->lb[d] ? g->ub[d] - g->lb[d] : 0;
  const char* min_cells_env = getenv("NEPTUNE_HIP_CHAIN_MIN_CELLS");
  const int64_t min_cells = min_cells_env ? atoll(min_cells_env) : (int64_t)4000000;
  return cells >= min_cells && !getenv("NEPTUNE_HIP_NO_PAIRS");
}

// the grouping to start with, per (entries, geometry) and process; 0 = the largest grouping's entry refused this geometry:
// single launches from now on
struct Choice { neptune_hip_apply_fn fn; int body; group_fn more[2]; neptune_hip_apply_geom_t g; int best; };
std::vector<Choice> g_choices;
std::mutex g_choice_mu;
// caller holds g_choice_mu
Choice* find_choice(const LoopKey& k) {
  for (Choice& c : g_choices)
    if (c.fn == k.fn && c.body == k.body && c.more[0] == k.more[0] && c.more[1] == k.more[1] && memcmp(&c.g, &k.g, sizeof(k.g)) == 0)
      return &c;
  return nullptr;
}
void remember_grouping(const LoopKey& k, int best) {
  std::lock_guard<std::mutex> lk(g_choice_mu);
  if (Choice* c = find_choice(k)) c->best = best;
  else g_choices.push_back({k.fn, k.body, {k.more[0], k.more[1]}, k.g, best});
}

// How many steps per launch (1 .. largest) the loop should try first, where grouping_allowed().  Whether grouping pays for
// THIS body is measured, once per (entries, geometry) and process: a Laplacian gains 1.7-2.4x from chaining, a 13-point
// operator 1.1x on its 3x8 window, a body heavy enough to be bound by its arithmetic loses (the windows overlap: every stage
// computes 1.3-1.8x the cells it keeps).  Each grouping the entries offer runs once to warm and twice under HIP events, from
// state `s0` into the buffers that the loop's first launch overwrites anyway.  Not measured (then: the largest grouping)
// unless `measure` -- the loop is long enough and tuning is on -- and not under stream capture.
// measure: the caller's business because the two loops read NEPTUNE_HIP_TUNE differently on purpose -- the one-level loop
// through the process-wide cached tune_mode(), the leapfrog loop on every call (its callers flip it within one process).
// refusal_is_final: NEPTUNE_HIP_EUNSUPPORTED from the largest grouping's trial is remembered as 0 (the leapfrog loop; the
// one-level loop has a middle grouping left to try).
template <class State, class Launch>
int choose_grouping(const LoopKey& key, const StreamScope& sc, bool measure, int largest, bool refusal_is_final, const State& s0,
                    Launch&& launch) {
  int known = -1;
  {
    std::lock_guard<std::mutex> lk(g_choice_mu);
    if (const Choice* c = find_choice(key)) known = c->best;
  }
  if (known == 0) return 1;
  if (!measure) return largest;
  if (known > 0) return known;
  if (sc.capturing) return largest;
  hipEvent_t e0, e1;
  NEPTUNE_HIP_CHECK(hipEventCreate(&e0));
  NEPTUNE_HIP_CHECK(hipEventCreate(&e1));
  int best = largest;
  double best_ms = -1;
  bool refused = false;
  for (int kind = 1; kind <= largest; ++kind) {
    auto one = [&] { State t = s0; return launch(kind, t); };
    const int rc = one();
    if (rc != NEPTUNE_HIP_OK) {   // a grouping these entries / this geometry do not offer
      refused = refusal_is_final && kind == largest && rc == NEPTUNE_HIP_EUNSUPPORTED;
      continue;
    }
    NEPTUNE_HIP_CHECK(hipEventRecord(e0, sc.stream));
    (void)one();
    (void)one();
    NEPTUNE_HIP_CHECK(hipEventRecord(e1, sc.stream));
    NEPTUNE_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    NEPTUNE_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double per_step = ms / (2.0 * kind);
    if (best_ms < 0 || per_step < 0.97 * best_ms) { best_ms = per_step; best = kind; }   // a larger grouping must win by 3 %
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  remember_grouping(key, refused ? 0 : best);
  return best;
}

int64_t g_leap_counts[2] = {0, 0};   // single / pair launches of the last leapfrog loop
int64_t g_system_counts[2] = {0, 0}; // steps / graph launches of the last system loop
void* g_until_sum = nullptr;            // the until loop's device scalar (one element), released with the graphs
int64_t g_until_counts[3] = {0, 0, 0};  // monitored checked steps / fallback checked steps / checks of the last until loop
void* g_cg_ws = nullptr;                // the solver's device block: CgScalars / PcgScalars / BicgScalars, then the partials of its own kernels; grown on demand
size_t g_cg_ws_bytes = 0;
int64_t g_cg_counts[3] = {0, 0, 0};     // dot-monitored iterations / fallback iterations / checks of the last cg_solve / pcg_solve / bicgstab_solve
double g_pcg_rz0 = 0.0;                 // r . (minv r) after the set-up of the last pcg_solve
constexpr size_t kCgScalarBytes = 64;   // room for CgScalars<double> and PcgScalars<double>, keeps the partials 16-byte aligned
constexpr size_t kBicgScalarBytes = 96; // BiCGStab's own reserve in the same block: BicgScalars<double> is 80 bytes; a multiple of 16 likewise
static_assert(sizeof(CgScalars<double>) <= kCgScalarBytes && sizeof(PcgScalars<double>) <= kCgScalarBytes &&
              sizeof(BicgScalars<double>) <= kBicgScalarBytes && kCgScalarBytes % 16 == 0 && kBicgScalarBytes % 16 == 0,
              "the scalar block");

// ---------------------------------------------------------------- the one-level loop on a stream scope
// `steps` applies from fields[0] (the state) into fields[steps % 2]: what neptune_hip_step_loop_chain is once its arguments
// are checked, and what neptune_hip_step_loop_until runs between two checks.
int one_level_loop(const StreamScope& sc, neptune_hip_apply_fn fn, neptune_hip_apply_fn fn2, neptune_hip_apply_fn fn3, int body,
                   const neptune_hip_apply_geom_t* g, void* const fields[2], const void* const* in, int64_t steps,
                   const neptune_hip_launch_cfg_t* cfg) {
  if (steps == 0) return NEPTUNE_HIP_OK;
  const neptune_hip_apply_fn chain[2] = {fn ? fn2 : nullptr, fn ? fn3 : nullptr};
  LoopKey key;
  init_key(key, fn, fn ? -1 : body, g, cfg, sc.stream);
  key.more[0] = (group_fn)chain[0];
  key.more[1] = (group_fn)chain[1];
  key.fields[0] = fields[0];
  key.fields[1] = fields[1];
  for (int i = 1; i < g->num_inputs; ++i) key.in[i] = in[i];

  // one launch of `applies` chained applies (1 = the plain apply) from fields[from] into the other field, which then holds
  // the state; a grouping the body or the geometry does not allow returns NEPTUNE_HIP_EUNSUPPORTED
  auto launch = [&](int applies, int& from) -> int {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    loop_inputs(key, ins, from, -1);
    const neptune_hip_launch_cfg_t* c = loop_cfg(key);
    void* out = key.fields[from ^ 1];
    int rc;
    if (applies == 1)
      rc = fn ? fn(&key.g, ins, out, (void*)sc.stream, c) : neptune_hip_apply_builtin(key.body, &key.g, ins, out, (void*)sc.stream, c);
    else if (c && (c->kernel == NEPTUNE_HIP_KERNEL_DIRECT || c->variant >= 0))
      rc = NEPTUNE_HIP_EUNSUPPORTED;   // an explicit tile was asked for
    else if (fn)
      rc = chain[applies - 2] ? chain[applies - 2](&key.g, ins, out, (void*)sc.stream, c) : NEPTUNE_HIP_EUNSUPPORTED;
    else
      rc = neptune_hip_apply_chain_builtin(key.body, applies, &key.g, ins, out, (void*)sc.stream, c);
    if (rc == NEPTUNE_HIP_OK) from ^= 1;
    return rc;
  };
  int from = 0;
  // graphs of 8 ping-pong pairs (the rotation's period is 2): 16 kernel nodes amortise one graph launch
  auto run = [&](int applies, int64_t count) { return replay(key, sc, applies, count, from, 16, launch); };

  // Several steps per pass over HBM.  Every launch -- of one, two or three chained applies -- moves the state to the other
  // field, and the newest state has to end in fields[steps % 2]:
  //   * triples: steps = 3 T + r needs T + r launches, and T + r = steps (mod 2) always: T triples, then r < 3 single steps;
  //   * pairs (when the triple entry does not exist or refuses): an EVEN number of pair launches brings the state back to
  //     fields[0], the remaining < 4 steps run as single launches.
  // The grouping does not change a bit: the same apply is evaluated, cell by cell, the same number of times on the same
  // operands.  NEPTUNE_HIP_NO_TRIPLES=1 stops at two applies per launch.
  const bool chain_ok = grouping_allowed(g), triples_ok = !getenv("NEPTUNE_HIP_NO_TRIPLES");
  const int best = chain_ok ? choose_grouping(key, sc, steps >= 8 && tune_mode() != 0, triples_ok ? 3 : 2, false, from, launch) : 1;
  if (steps >= 3 && best >= 3 && triples_ok) {
    const int64_t triples = steps / 3;
    const int rc3 = run(3, triples);
    if (rc3 == NEPTUNE_HIP_OK) return run(1, steps - 3 * triples);
    if (rc3 != NEPTUNE_HIP_EUNSUPPORTED) return rc3;
  }
  if (steps >= 4 && best >= 2) {
    const int64_t pairs = (steps / 2) & ~(int64_t)1;
    const int rc2 = run(2, pairs);
    if (rc2 == NEPTUNE_HIP_OK) return run(1, steps - 2 * pairs);
    if (rc2 != NEPTUNE_HIP_EUNSUPPORTED) return rc2;
  }
  return run(1, steps);
}

}  // namespace

namespace neptune_hip {
// for neptune_hip_finalize (solver_host.hpp; not exported)
void step_loop_destroy_graphs() {
  std::lock_guard<std::mutex> lk(g_loop_mu);
  for (auto& e : g_loops) {
    destroy_graph(e);
    e.stamp = 0;
  }
  if (g_until_sum) {
    (void)hipFree(g_until_sum);
    g_until_sum = nullptr;
  }
  if (g_cg_ws) {
    (void)hipFree(g_cg_ws);
    g_cg_ws = nullptr;
    g_cg_ws_bytes = 0;
  }
}
}  // namespace neptune_hip

extern "C" {

// ---------------------------------------------------------------- one-level loop: two fields, ping-pong
int neptune_hip_step_loop(neptune_hip_apply_fn fn, int body, const neptune_hip_apply_geom_t* g, void* const fields[2],
                          const void* const* in, int64_t steps, void* stream, const neptune_hip_launch_cfg_t* cfg) {
  return neptune_hip_step_loop_pairs(fn, nullptr, body, g, fields, in, steps, stream, cfg);
}

int neptune_hip_step_loop_pairs(neptune_hip_apply_fn fn, neptune_hip_apply_fn fn2, int body, const neptune_hip_apply_geom_t* g,
                                void* const fields[2], const void* const* in, int64_t steps, void* stream,
                                const neptune_hip_launch_cfg_t* cfg) {
  return neptune_hip_step_loop_chain(fn, fn2, nullptr, body, g, fields, in, steps, stream, cfg);
}

int neptune_hip_step_loop_chain(neptune_hip_apply_fn fn, neptune_hip_apply_fn fn2, neptune_hip_apply_fn fn3, int body,
                                const neptune_hip_apply_geom_t* g, void* const fields[2], const void* const* in, int64_t steps,
                                void* stream, const neptune_hip_launch_cfg_t* cfg) {
  if (!g || !fields || !fields[0] || !fields[1] || fields[0] == fields[1] || steps < 0) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs < 1 || g->num_inputs > NEPTUNE_HIP_MAX_INPUTS) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs > 1 && !in) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  if (steps == 0) return NEPTUNE_HIP_OK;
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  return one_level_loop(sc, fn, fn2, fn3, body, g, fields, in, steps, cfg);
}

// ---------------------------------------------------------------- iteration to a tolerance: the one-level loop in blocks
void neptune_hip_until_loop_counts(int64_t* fused, int64_t* fallback, int64_t* checks) {
  if (fused) *fused = g_until_counts[0];
  if (fallback) *fallback = g_until_counts[1];
  if (checks) *checks = g_until_counts[2];
}

int neptune_hip_step_loop_until(neptune_hip_apply_fn fn, neptune_hip_apply_norm_fn fn_norm, int body, int dtype_of_fn,
                                const neptune_hip_apply_geom_t* g, void* const fields[2], const void* const* in, int64_t max_steps,
                                int64_t check_every, double tol2, void* stream, const neptune_hip_launch_cfg_t* cfg,
                                int64_t* steps_done, double* last_sum) {
  g_until_counts[0] = g_until_counts[1] = g_until_counts[2] = 0;
  if (steps_done) *steps_done = 0;
  if (last_sum) *last_sum = 0.0;
  if (!g || !fields || !fields[0] || !fields[1] || fields[0] == fields[1] || max_steps < 0 || check_every < 1) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs < 1 || g->num_inputs > NEPTUNE_HIP_MAX_INPUTS) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs > 1 && !in) return NEPTUNE_HIP_EINVAL;
  int dtype = 0;
  if (!entry_dtype(fn, body, dtype_of_fn, &dtype)) return NEPTUNE_HIP_EINVAL;
  // the scalar is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  if (max_steps == 0) return NEPTUNE_HIP_OK;
  if (!g_until_sum) NEPTUNE_HIP_CHECK(hipMalloc(&g_until_sum, 8));
  void* const sum_dev = g_until_sum;
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  const neptune_hip_launch_cfg_t* c = set_cfg(cfg);
  bool fused_ok = fn ? fn_norm != nullptr : true;   // false once the monitored entry has refused this geometry
  int64_t done = 0;
  int cur = 0;   // fields[cur] holds the state
  double sum = 0.0;
  while (done < max_steps) {
    const int64_t block = check_every < max_steps - done ? check_every : max_steps - done;
    // the block's first steps: intermediate states are not needed, so graphs and chained launches apply as in any loop
    if (block > 1) {
      void* const fl[2] = {fields[cur], fields[cur ^ 1]};
      const int rc = one_level_loop(sc, fn, nullptr, nullptr, body, g, fl, in, block - 1, cfg);
      if (rc != NEPTUNE_HIP_OK) return rc;
      cur ^= (int)((block - 1) & 1);
      done += block - 1;
      if (steps_done) *steps_done = done;
    }
    // the block's last step, checked
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    for (int i = 1; i < g->num_inputs; ++i) ins[i] = in[i];
    ins[0] = fields[cur];
    void* const out = fields[cur ^ 1];
    int rc = NEPTUNE_HIP_EUNSUPPORTED;
    if (fused_ok) {
      rc = fn ? fn_norm(g, ins, out, sum_dev, (void*)sc.stream, c) : neptune_hip_apply_builtin_norm(body, g, ins, out, sum_dev, (void*)sc.stream, c);
      if (rc == NEPTUNE_HIP_OK) ++g_until_counts[0];
      else if (rc == NEPTUNE_HIP_EUNSUPPORTED) fused_ok = false;   // nothing was launched: the fallback, now and for the rest of the call
      else return rc;
    }
    if (rc == NEPTUNE_HIP_EUNSUPPORTED) {
      rc = fn ? fn(g, ins, out, (void*)sc.stream, c) : neptune_hip_apply_builtin(body, g, ins, out, (void*)sc.stream, c);
      if (rc != NEPTUNE_HIP_OK) return rc;
      rc = neptune_hip_update_norm(dtype, g, out, ins[0], sum_dev, (void*)sc.stream);
      if (rc != NEPTUNE_HIP_OK) return rc;
      ++g_until_counts[1];
    }
    cur ^= 1;
    ++done;
    if (steps_done) *steps_done = done;
    read_scalars(dtype, sc.stream, sum_dev, 1, &sum);
    ++g_until_counts[2];
    if (last_sum) *last_sum = sum;
    if (sum <= tol2) break;   // false for a NaN sum: such a loop runs to max_steps
  }
  return NEPTUNE_HIP_OK;
}

// ---------------------------------------------------------------- leapfrog loop (two-level schemes): three or four fields
void neptune_hip_leapfrog_launch_counts(int64_t* singles, int64_t* pairs) {
  if (singles) *singles = g_leap_counts[0];
  if (pairs) *pairs = g_leap_counts[1];
}

int neptune_hip_step_loop_leapfrog(neptune_hip_apply_fn fn, neptune_hip_leapfrog2_fn fn2, const neptune_hip_apply_geom_t* g,
                                   void* const fields[4], const void* const* extra, int n_extra, int64_t steps, void* stream,
                                   const neptune_hip_launch_cfg_t* cfg, int* cur, int* prev) {
  if (!fn || !g || !fields || !fields[0] || !fields[1] || !fields[2] || steps < 0 || n_extra < 0) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs != 2 + n_extra || g->num_inputs > NEPTUNE_HIP_MAX_INPUTS || (n_extra > 0 && !extra)) return NEPTUNE_HIP_EINVAL;
  const int nf = fields[3] ? 4 : 3;
  for (int a = 0; a < nf; ++a)
    for (int b = a + 1; b < nf; ++b)
      if (fields[a] == fields[b]) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  g_leap_counts[0] = g_leap_counts[1] = 0;
  LeapState st = {0, 1, 2, fields[3] ? 3 : -1};
  auto result = [&](int rc) {
    if (cur) *cur = st.cur;
    if (prev) *prev = st.prev;
    return rc;
  };
  if (steps == 0) return result(NEPTUNE_HIP_OK);
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  LoopKey key;
  init_key(key, fn, -1, g, cfg, sc.stream);
  key.more[0] = (group_fn)fn2;
  for (int a = 0; a < 4; ++a) key.fields[a] = fields[a];
  for (int i = 0; i < n_extra; ++i) key.in[2 + i] = extra[i];

  // one launch of `kind` steps (1: the apply itself into f1; 2: the pair entry into (f1, f2)) and the rotation after it:
  //   single: (prev, cur, f1) <- (cur, f1, prev)                 -- period 3
  //   pair:   (prev, cur) <- (v, w) = (f1, f2), (f1, f2) <- (old prev, old cur)   -- period 2
  auto launch = [&](int kind, LeapState& s) -> int {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    loop_inputs(key, ins, s.cur, s.prev);
    if (kind == 1) {
      const int rc = fn(&key.g, ins, key.fields[s.f1], (void*)sc.stream, loop_cfg(key));
      if (rc == NEPTUNE_HIP_OK) s = {s.f1, s.cur, s.prev, s.f2};
      return rc;
    }
    const int rc = fn2(&key.g, ins, key.fields[s.f1], key.fields[s.f2], (void*)sc.stream, loop_cfg(key));
    if (rc == NEPTUNE_HIP_OK) s = {s.f2, s.f1, s.prev, s.cur};
    return rc;
  };
  // ONE linear chain per graph, a multiple of the rotation's period: 18 single or 8 pair launches
  auto run = [&](int kind, int64_t count) {
    const int rc = replay(key, sc, kind, count, st, kind == 1 ? 18 : 8, launch);
    if (rc == NEPTUNE_HIP_OK && count > 0) g_leap_counts[kind - 1] += count;
    return rc;
  };

  // steps / 2 pairs, then at most one single launch -- where pairs are allowed and chosen; single launches otherwise.
  // NEPTUNE_HIP_TUNE is read on every call here.
  const char* tune_env = getenv("NEPTUNE_HIP_TUNE");
  const bool tune = !(tune_env && *tune_env == '0');
  const bool pairs_ok = fn2 && fields[3] && steps >= 2 && grouping_allowed(g);
  if (pairs_ok && choose_grouping(key, sc, steps >= 8 && tune, 2, true, st, launch) >= 2) {
    const int64_t pairs = steps / 2;
    const int rc2 = run(2, pairs);
    if (rc2 == NEPTUNE_HIP_OK) return result(run(1, steps - 2 * pairs));
    if (rc2 != NEPTUNE_HIP_EUNSUPPORTED) return result(rc2);
    remember_grouping(key, 0);   // nothing has run: single launches, now and for the rest of the process
  }
  return result(run(1, steps));
}

// ---------------------------------------------------------------- system loop: a group's n_out unknowns, two sets of fields
void neptune_hip_system_loop_counts(int64_t* launches, int64_t* graph_launches) {
  if (launches) *launches = g_system_counts[0];
  if (graph_launches) *graph_launches = g_system_counts[1];
}

int neptune_hip_step_loop_system(neptune_hip_group_fn fn, const neptune_hip_apply_geom_t* g, int n_out, const int* through,
                                 void* const* fields_a, void* const* fields_b, const void* const* in, int64_t steps, void* stream,
                                 const neptune_hip_launch_cfg_t* cfg) {
  g_system_counts[0] = g_system_counts[1] = 0;
  if (!fn || !g || !through || !fields_a || !fields_b || steps < 0 || n_out < 2 || n_out > 4) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs < n_out || g->num_inputs > NEPTUNE_HIP_MAX_INPUTS) return NEPTUNE_HIP_EINVAL;
  bool advanced[NEPTUNE_HIP_MAX_INPUTS] = {};
  for (int m = 0; m < n_out; ++m) {
    // two members advancing the same unknown is not a time step
    if (through[m] < 0 || through[m] >= g->num_inputs || advanced[through[m]]) return NEPTUNE_HIP_EINVAL;
    advanced[through[m]] = true;
  }
  const void* bufs[8];
  for (int m = 0; m < n_out; ++m) { bufs[m] = fields_a[m]; bufs[n_out + m] = fields_b[m]; }
  for (int a = 0; a < 2 * n_out; ++a) {
    if (!bufs[a]) return NEPTUNE_HIP_EINVAL;
    for (int b = 0; b < a; ++b)
      if (bufs[a] == bufs[b]) return NEPTUNE_HIP_EINVAL;
  }
  for (int k = 0; k < g->num_inputs; ++k)
    if (!advanced[k] && (!in || !in[k])) return NEPTUNE_HIP_EINVAL;   // a fixed input is missing
  ensure_init();
  if (steps == 0) return NEPTUNE_HIP_OK;
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  LoopKey key;
  init_key(key, nullptr, -1, g, cfg, sc.stream);
  key.more[0] = (group_fn)fn;
  key.n_out = n_out;
  for (int m = 0; m < n_out; ++m) {
    key.fields[m] = fields_a[m];
    key.fields_b[m] = fields_b[m];
    key.through[m] = through[m];
  }
  for (int k = 0; k < g->num_inputs; ++k)
    if (!advanced[k]) key.in[k] = in[k];

  // one step: every member reads set `from` (0 = A) at its unknown's input and writes the other set
  auto launch = [&](int, int& from) -> int {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    void* outs[4];
    for (int k = 0; k < key.g.num_inputs; ++k) ins[k] = key.in[k];
    for (int m = 0; m < key.n_out; ++m) {
      ins[key.through[m]] = from ? key.fields_b[m] : key.fields[m];
      outs[m] = from ? key.fields[m] : key.fields_b[m];
    }
    const int rc = fn(&key.g, ins, outs, (void*)sc.stream, loop_cfg(key));
    if (rc == NEPTUNE_HIP_OK) from ^= 1;
    return rc;
  };
  // one launch kind, no grouping to choose: graphs of 8 ping-pong pairs, as the one-level loop's
  int from = 0;
  const int rc = replay(key, sc, 1, steps, from, 16, launch, &g_system_counts[1]);
  if (rc == NEPTUNE_HIP_OK) g_system_counts[0] = steps;
  return rc;
}

}  // extern "C"

// ---------------------------------------------------------------- the Krylov solvers on a stream scope
namespace {
// the solvers' device block holds at least `need` bytes from here on
void grow_cg_ws(size_t need, hipStream_t stream) {
  if (need <= g_cg_ws_bytes) return;
  std::lock_guard<std::mutex> lk(g_loop_mu);   // cached graphs hold the old block's address: their keys do too
  if (g_cg_ws) {
    NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
    NEPTUNE_HIP_CHECK(hipFree(g_cg_ws));
  }
  g_cg_ws = nullptr;
  g_cg_ws_bytes = 0;
  NEPTUNE_HIP_CHECK(hipMalloc(&g_cg_ws, need));
  g_cg_ws_bytes = need;
}

// the box all of a solver's fields share, and Omega in its physical coordinates, on the kernels' (I, J, K) axes; -> the cells
// of the box
int64_t solver_box(const neptune_hip_apply_geom_t* g, CgBoxParams& B) {
  int64_t n = 1;
  int64_t shape[3], lo[3], hi[3];
  for (int d = 0; d < g->rank; ++d) {
    shape[d] = g->out_ub[d] - g->out_lb[d];
    lo[d] = std::max(g->lb[d] - g->out_lb[d], g->region_lb[d]);
    hi[d] = std::min(g->ub[d] - g->out_lb[d], g->region_ub[d]);
    n *= shape[d];
  }
  auto axes = [&](const int64_t* src, int64_t* dst, int64_t fill) {
    if (g->rank == 3) to_axes<3>(src, dst, fill);
    else if (g->rank == 2) to_axes<2>(src, dst, fill);
    else to_axes<1>(src, dst, fill);
  };
  axes(shape, B.n, 1);
  axes(lo, B.lo, 0);
  axes(hi, B.hi, 1);
  return n;
}
// a solver entry's arguments once they are checked (include/neptune_hip.h); minv: nullptr unless neptune_hip_pcg_solve
struct SolveArgs {
  neptune_hip_apply_fn fn;
  neptune_hip_apply_dot_fn fn_dot;
  int body;
  const neptune_hip_apply_geom_t* g;
  void* x;
  const void* b;
  const void* minv;
  void* const* work;
  const void* const* in_rest;
  int64_t max_iters, check_every;
  double tol2;
  void* trace;
  const neptune_hip_launch_cfg_t* cfg;
  int64_t* iters_done;
  double* rr0;
  double* rr_last;
};

// What the host loops of all solvers share: the box and the set-up grid, the operator A (solver_host.hpp), the common part of
// the graph key and the schedule -- blocks of check_every iterations, each replayed through the engine, r . r read back after
// each.  A solver is its set-up, its `iteration` and one call of run().
template <class T>
struct SolverFrame {
  const StreamScope& sc;
  const SolveArgs& a;
  const OuterOperator A;
  CgBoxParams B;
  int64_t n, nchunk, init_blocks;
  dim3 init_grid;
  bool fused_ok;   // false once the dot-monitored entry has refused this geometry

  SolverFrame(const StreamScope& sc_, const SolveArgs& a_)
      : sc(sc_), a(a_), A{a_.fn, a_.fn_dot, a_.body, a_.g, a_.in_rest, set_cfg(a_.cfg), sc_.stream}, fused_ok(A.has_dot()) {
    n = solver_box(a.g, B);
    nchunk = (B.n[2] + 255) / 256;
    init_grid = grid_for_blocks(B.n[0] * B.n[1] * nchunk);
    init_blocks = (int64_t)init_grid.x * init_grid.y;
  }
  // the part of the graph key every solver fills alike; n_out < 0 tells the solvers' keys from every loop's and from each other's
  void init_solver_key(LoopKey& key, int n_out) const {
    init_key(key, a.fn, a.fn ? -1 : a.body, a.g, a.cfg, sc.stream);
    key.n_out = n_out;
    key.more[0] = (group_fn)a.fn_dot;
    key.fields_b[0] = g_cg_ws;
    key.fields_b[2] = a.trace;
    key.through[0] = (int)(a.max_iters < 0x7fffffff ? a.max_iters : 0x7fffffff);   // the trace's length is a kernel argument
    for (int i = 1; i < a.g->num_inputs; ++i) key.in[i] = a.in_rest[i - 1];
  }
  // The schedule.  iteration(kind, state): kind 1 uses the dot-monitored launch, kind 2 the fallback; graphs of `per_graph`
  // iterations (about 40 kernel nodes, as the other loops amortise a graph launch over 16 applies).
  // retry_on_refusal (CG, whose iteration BEGINS with the dot-monitored launch): NEPTUNE_HIP_EUNSUPPORTED from a block comes
  // from its first launch alone (replay), so nothing of the block has run; the block runs again as kind 2, as does the rest
  // of the call.  Without it (BiCGStab, which asks the entry once before its first iteration) a refusal is an error.
  template <class Iteration>
  int run(LoopKey& key, const T* rr_dev, int per_graph, bool retry_on_refusal, Iteration&& iteration) {
    int64_t done = 0;
    int state = 0;   // an iteration leaves no rotation behind: the device block carries it
    while (done < a.max_iters) {
      const int64_t block = a.check_every < a.max_iters - done ? a.check_every : a.max_iters - done;
      int rc = replay(key, sc, fused_ok ? 1 : 2, block, state, per_graph, iteration);
      if (retry_on_refusal) {
        if (rc == NEPTUNE_HIP_EUNSUPPORTED && fused_ok) {
          fused_ok = false;
          rc = replay(key, sc, 2, block, state, per_graph, iteration);
        }
        if (rc != NEPTUNE_HIP_OK) return rc;
      } else if (rc != NEPTUNE_HIP_OK) {
        return late(rc);
      }
      g_cg_counts[fused_ok ? 0 : 1] += block;
      done += block;
      if (a.iters_done) *a.iters_done = done;
      double rr;
      read_scalars(sc.stream, rr_dev, 1, &rr);
      ++g_cg_counts[2];
      if (a.rr_last) *a.rr_last = rr;
      if (rr <= a.tol2) break;   // false for a NaN: such a solve runs to max_iters
    }
    return NEPTUNE_HIP_OK;
  }
};
// minv = nullptr: the solver of 3.11; a field: the Jacobi-preconditioned solver of 3.12 on its own kernels and scalar block
template <class T>
int cg_solve_typed(const StreamScope& sc, const SolveArgs& a) {
  SolverFrame<T> S(sc, a);
  const int dtype = sizeof(T) == 8 ? NEPTUNE_HIP_F64 : NEPTUNE_HIP_F32;
  T* const x = static_cast<T*>(a.x);
  T* const r = static_cast<T*>(a.work[0]);
  T* const p = static_cast<T*>(a.work[1]);
  T* const q = static_cast<T*>(a.work[2]);
  const T* const b = static_cast<const T*>(a.b);
  const T* const minv = static_cast<const T*>(a.minv);
  const int64_t n = S.n;
  // (a null minv is 16-byte aligned: it does not decide the form)
  const FlatGrid upd = flat_grid(n, sizeof(T), {p, q, x, r, minv}), dir = flat_grid(n, sizeof(T), {r, p, minv});

  // the device block: the scalars, then room for the partials of the init and update kernels (two sums with a preconditioner)
  grow_cg_ws(kCgScalarBytes + (size_t)(minv ? 2 : 1) * (size_t)std::max<int64_t>(S.init_blocks, upd.blocks) * sizeof(T), sc.stream);
  CgScalars<T>* const scal = static_cast<CgScalars<T>*>(g_cg_ws);
  PcgScalars<T>* const pscal = static_cast<PcgScalars<T>*>(g_cg_ws);   // the same bytes: one of the two is in use
  T* const pq_dev = minv ? &pscal->pq : &scal->pq;
  T* const partials = reinterpret_cast<T*>(static_cast<char*>(g_cg_ws) + kCgScalarBytes);
  T* const tr = static_cast<T*>(a.trace);
  // the one-workgroup kernel after the init kernel (start) or after the update kernel
  auto final_kernel = [&](int64_t count, T* trace, int64_t trace_iters, bool start) {
    if (minv) hipLaunchKernelGGL(neptune_pcg_final<T>, dim3(1), dim3(256), 0, sc.stream, (const T*)partials, count, pscal, trace, trace_iters, start);
    else hipLaunchKernelGGL(neptune_cg_final<T>, dim3(1), dim3(256), 0, sc.stream, (const T*)partials, count, scal, trace, trace_iters, start);
  };

  // set-up: q = A(x), r = p = b - q on Omega, rr_0.  An apply stores nothing outside its launch region, and the flat update
  // reads q everywhere: where the region is not the whole box, q starts as +0 and stays so out there.
  if (!region_is_whole(a.g)) NEPTUNE_HIP_CHECK(hipMemsetAsync(q, 0, (size_t)n * sizeof(T), sc.stream));
  const int rc = S.A.apply(x, q);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (minv) hipLaunchKernelGGL(neptune_pcg_init<T>, S.init_grid, dim3(256), 0, sc.stream, S.B, S.nchunk, S.init_blocks, b, (const T*)q, minv, r, p, partials);
  else hipLaunchKernelGGL(neptune_cg_init<T>, S.init_grid, dim3(256), 0, sc.stream, S.B, S.nchunk, b, (const T*)q, r, p, partials);
  final_kernel(S.init_blocks, nullptr, 0, true);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  double h[2];
  if (minv) {   // rz_0 and rr_0 lie side by side
    read_scalars(sc.stream, &pscal->rz, 2, h);
    g_pcg_rz0 = h[0];
  } else {
    read_scalars(sc.stream, &scal->rr, 1, &h[1]);
  }
  if (done_after_setup(h[1], a.tol2, a.max_iters, a.rr0, a.rr_last)) return NEPTUNE_HIP_OK;

  LoopKey key;
  S.init_solver_key(key, -1);
  key.fields[0] = x; key.fields[1] = r; key.fields[2] = p; key.fields[3] = q;
  key.fields_b[3] = const_cast<T*>(minv);   // a graph captured with one preconditioner is never replayed with another

  // one iteration; kind 1: q = A(p) and pq out of one dot-monitored launch, kind 2: a plain launch and neptune_hip_dot.
  // NEPTUNE_HIP_EUNSUPPORTED comes from the dot-monitored entry alone, which then has launched nothing.
  auto iteration = [&](int kind, int&) -> int {
    int rc;
    if (kind == 1) {
      rc = S.A.apply_dot(p, q, pq_dev);
      if (rc != NEPTUNE_HIP_OK) return rc;
      key.fields_b[1] = neptune_hip_monitor_workspace(0, (void*)sc.stream);   // where that launch's partials live: part of a graph
    } else {
      rc = S.A.apply(p, q);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      rc = neptune_hip_dot(dtype, a.g, q, p, pq_dev, (void*)sc.stream);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
    }
    if (minv) flat_launch(upd, sc.stream, neptune_pcg_update<T, true>, neptune_pcg_update<T, false>, n, pscal, p, q, minv, x, r, partials);
    else flat_launch(upd, sc.stream, neptune_cg_update<T, true>, neptune_cg_update<T, false>, n, scal, p, q, x, r, partials);
    final_kernel((int64_t)upd.blocks, tr, a.max_iters, false);
    if (minv) flat_launch(dir, sc.stream, neptune_pcg_direction<T, true>, neptune_pcg_direction<T, false>, n, pscal, r, minv, p);
    else flat_launch(dir, sc.stream, neptune_cg_direction<T, true>, neptune_cg_direction<T, false>, n, scal, r, p);
    NEPTUNE_HIP_CHECK(hipGetLastError());
    return NEPTUNE_HIP_OK;
  };
  return S.run(key, minv ? &pscal->rr : &scal->rr, 8, true, iteration);
}

// BiCGStab (3.13): other vectors, other kernels and three reduction points per iteration on the same frame
template <class T>
int bicgstab_solve_typed(const StreamScope& sc, const SolveArgs& a) {
  SolverFrame<T> S(sc, a);
  T* const x = static_cast<T*>(a.x);
  T* const r = static_cast<T*>(a.work[0]);    // s between the two half-steps
  T* const rh = static_cast<T*>(a.work[1]);
  T* const p = static_cast<T*>(a.work[2]);
  T* const v = static_cast<T*>(a.work[3]);
  T* const t = static_cast<T*>(a.work[4]);
  const int64_t n = S.n;
  const FlatGrid g_rv = flat_grid(n, sizeof(T), {rh, v}), g_s = flat_grid(n, sizeof(T), {v, r}),
                 g_tt = flat_grid(n, sizeof(T), {t}), g_ts = flat_grid(n, sizeof(T), {t, r}),
                 g_upd = flat_grid(n, sizeof(T), {p, t, rh, x, r}), g_dir = flat_grid(n, sizeof(T), {r, v, p});
  // the device block: the scalars, then room for the partials of the init, sum and update kernels (two sums at the most)
  const int64_t most = std::max<int64_t>({S.init_blocks, g_rv.blocks, g_tt.blocks, g_ts.blocks, g_upd.blocks});
  grow_cg_ws(kBicgScalarBytes + 2 * (size_t)most * sizeof(T), sc.stream);
  BicgScalars<T>* const scal = static_cast<BicgScalars<T>*>(g_cg_ws);
  T* const partials = reinterpret_cast<T*>(static_cast<char*>(g_cg_ws) + kBicgScalarBytes);
  auto final_kernel = [&](int64_t count, int stage) {
    hipLaunchKernelGGL(neptune_bicg_final<T>, dim3(1), dim3(256), 0, sc.stream, (const T*)partials, count, scal, static_cast<T*>(a.trace), a.max_iters, stage);
  };

  // set-up: v = A(x), r = rh = p = b - v on Omega, rr_0 = rho_0.  An apply stores nothing outside its launch region, and the
  // flat kernels read v and t everywhere: where the region is not the whole box, both start as +0 and stay so out there.
  if (!region_is_whole(a.g)) {
    NEPTUNE_HIP_CHECK(hipMemsetAsync(v, 0, (size_t)n * sizeof(T), sc.stream));
    NEPTUNE_HIP_CHECK(hipMemsetAsync(t, 0, (size_t)n * sizeof(T), sc.stream));
  }
  int rc = S.A.apply(x, v);
  if (rc != NEPTUNE_HIP_OK) return rc;
  hipLaunchKernelGGL(neptune_bicg_init<T>, S.init_grid, dim3(256), 0, sc.stream, S.B, S.nchunk, static_cast<const T*>(a.b), (const T*)v, r, rh, p, partials);
  final_kernel(S.init_blocks, kBicgStart);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  double rr;
  read_scalars(sc.stream, &scal->rr, 1, &rr);
  if (done_after_setup(rr, a.tol2, a.max_iters, a.rr0, a.rr_last)) return NEPTUNE_HIP_OK;

  LoopKey key;
  S.init_solver_key(key, -2);
  key.fields[0] = x; key.fields[1] = r; key.fields[2] = p; key.fields[3] = v;
  key.fields_c[0] = rh; key.fields_c[1] = t; key.fields_c[2] = const_cast<void*>(a.b);

  // The dot-monitored entry is an iteration's FOURTH launch: a refusal from there would leave half an iteration behind.  So the
  // entry is asked once per call, before the first iteration, with the very launch step 3 makes (t = A(r) and ts, both of
  // which every iteration writes again before it reads them): a refusal -- NEPTUNE_HIP_EUNSUPPORTED, nothing launched -- is
  // remembered for the rest of the call, and an acceptance has grown the monitor workspace outside of any capture.
  if (S.fused_ok) {
    rc = S.A.apply_dot(r, t, &scal->ts);
    if (rc == NEPTUNE_HIP_EUNSUPPORTED) S.fused_ok = false;
    else if (rc != NEPTUNE_HIP_OK) return rc;
  }

  // one iteration; kind 1: t = A(s) and ts out of one dot-monitored launch, then tt; kind 2: a plain launch, then ts and tt out
  // of one pass
  auto iteration = [&](int kind, int&) -> int {
    // 1. v = A(p), rv = rh . v, alpha
    int rc = S.A.apply(p, v);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    flat_launch(g_rv, sc.stream, neptune_bicg_rv<T, true>, neptune_bicg_rv<T, false>, n, rh, v, partials);
    final_kernel((int64_t)g_rv.blocks, kBicgRv);
    // 2. s = r - alpha v, in place
    flat_launch(g_s, sc.stream, neptune_bicg_s<T, true>, neptune_bicg_s<T, false>, n, scal, v, r);
    NEPTUNE_HIP_CHECK(hipGetLastError());
    // 3. t = A(s), ts, tt, omega
    if (kind == 1) {
      rc = S.A.apply_dot(r, t, &scal->ts);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      key.fields_b[1] = neptune_hip_monitor_workspace(0, (void*)sc.stream);   // where that launch's partials live: part of a graph
      flat_launch(g_tt, sc.stream, neptune_bicg_tt<T, true, false>, neptune_bicg_tt<T, false, false>, n, t, t, partials);
      final_kernel((int64_t)g_tt.blocks, kBicgTt);
    } else {
      rc = S.A.apply(r, t);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      flat_launch(g_ts, sc.stream, neptune_bicg_tt<T, true, true>, neptune_bicg_tt<T, false, true>, n, t, r, partials);
      final_kernel((int64_t)g_ts.blocks, kBicgTsTt);
    }
    // 4. x, r, rho', rr', beta, the trace row and the rotation
    flat_launch(g_upd, sc.stream, neptune_bicg_update<T, true>, neptune_bicg_update<T, false>, n, scal, p, t, rh, x, r, partials);
    final_kernel((int64_t)g_upd.blocks, kBicgUpdate);
    // 5. p = r + beta (p - omega v)
    flat_launch(g_dir, sc.stream, neptune_bicg_direction<T, true>, neptune_bicg_direction<T, false>, n, scal, r, v, p);
    NEPTUNE_HIP_CHECK(hipGetLastError());
    return NEPTUNE_HIP_OK;
  };
  // graphs of 4 iterations: an iteration is 11 kernel nodes (10 on the fallback path) against CG's 5
  return S.run(key, &scal->rr, 4, false, iteration);
}
}  // namespace

extern "C" {

void neptune_hip_cg_counts(int64_t* fused, int64_t* fallback, int64_t* checks) {
  if (fused) *fused = g_cg_counts[0];
  if (fallback) *fallback = g_cg_counts[1];
  if (checks) *checks = g_cg_counts[2];
}

// The argument checks every solver shares, before anything touches the device: the scalars, the geometry, the fixed inputs,
// one box for input 0 and the result, the element type (-> *dtype_out), `count` non-null fields aligned for it and pairwise
// disjoint, a trace (of trace_values elements, or NULL) aligned and clear of every field, and no capture under way on `stream`.
static int solver_args_checked(neptune_hip_apply_fn fn, int body, int dtype_of_fn, const neptune_hip_apply_geom_t* g,
                               const void* const* fields, int count, const void* const* in_rest, int64_t max_iters, int64_t check_every,
                               const void* trace, int64_t trace_values, void* stream, int* dtype_out) {
  if (!g || max_iters < 0 || check_every < 1) return NEPTUNE_HIP_EINVAL;
  for (int a = 0; a < count; ++a)
    if (!fields[a]) return NEPTUNE_HIP_EINVAL;
  if (geom_validate(g) != NEPTUNE_HIP_OK) return NEPTUNE_HIP_EINVAL;
  if (g->num_inputs > 1 && !in_rest) return NEPTUNE_HIP_EINVAL;
  for (int i = 1; i < g->num_inputs; ++i)
    if (!in_rest[i - 1]) return NEPTUNE_HIP_EINVAL;
  // the iteration feeds the result back as input 0: one box for both
  for (int d = 0; d < g->rank; ++d)
    if (g->in_lb[0][d] != g->out_lb[d] || g->in_ub[0][d] != g->out_ub[d]) return NEPTUNE_HIP_EINVAL;
  int dtype = 0;
  if (!entry_dtype(fn, body, dtype_of_fn, &dtype)) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype);
  const size_t bytes = geom_box_bytes(g->out_lb, g->out_ub, g->rank, elem);
  const size_t trace_bytes = (size_t)trace_values * elem;
  for (int a = 0; a < count; ++a) {
    if ((uintptr_t)fields[a] % elem != 0) return NEPTUNE_HIP_EINVAL;
    for (int o = 0; o < a; ++o)
      if (buffers_overlap(fields[a], bytes, fields[o], bytes)) return NEPTUNE_HIP_EINVAL;
    if (trace && buffers_overlap(trace, trace_bytes, fields[a], bytes)) return NEPTUNE_HIP_EINVAL;
  }
  if (trace && (uintptr_t)trace % elem != 0) return NEPTUNE_HIP_EINVAL;
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;
  *dtype_out = dtype;
  return NEPTUNE_HIP_OK;
}

// The three entries' common path: counters and out-parameters zeroed, the arguments checked (x, b, the solver's n_work work
// fields and, where a.minv is set, minv as one more field; a trace of `cols` values per iteration), then the dispatch on the
// element type
enum Solver { kSolverCg, kSolverPcg, kSolverBicgstab };
static int solve_checked(Solver solver, int dtype_of_fn, void* stream, const SolveArgs& a) {
  g_cg_counts[0] = g_cg_counts[1] = g_cg_counts[2] = 0;
  reset_solver_outputs(a.iters_done, a.rr0, a.rr_last);
  if (!a.work) return NEPTUNE_HIP_EINVAL;
  const int n_work = solver == kSolverBicgstab ? 5 : 3;
  const int cols = solver == kSolverCg ? 2 : solver == kSolverPcg ? 3 : 5;
  const void* fields[8] = {a.x, a.b};
  int count = 2;
  for (int i = 0; i < n_work; ++i) fields[count++] = a.work[i];
  if (solver == kSolverPcg) fields[count++] = a.minv;
  int dtype = 0;
  if (solver_args_checked(a.fn, a.body, dtype_of_fn, a.g, fields, count, a.in_rest, a.max_iters, a.check_every, a.trace, cols * a.max_iters,
                          stream, &dtype) != NEPTUNE_HIP_OK)
    return NEPTUNE_HIP_EINVAL;
  ensure_init();
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  if (solver == kSolverBicgstab) return dtype == NEPTUNE_HIP_F64 ? bicgstab_solve_typed<double>(sc, a) : bicgstab_solve_typed<float>(sc, a);
  return dtype == NEPTUNE_HIP_F64 ? cg_solve_typed<double>(sc, a) : cg_solve_typed<float>(sc, a);
}

int neptune_hip_cg_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                         const neptune_hip_apply_geom_t* g, void* x, const void* b, void* const work[3], const void* const* in_rest,
                         int64_t max_iters, int64_t check_every, double tol2, void* trace, void* stream,
                         const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0, double* rr_last) {
  return solve_checked(kSolverCg, dtype_of_fn, stream,
                       {fn, fn_dot, body, g, x, b, nullptr, work, in_rest, max_iters, check_every, tol2, trace, cfg, iters_done, rr0, rr_last});
}

double neptune_hip_pcg_rz0(void) { return g_pcg_rz0; }

int neptune_hip_pcg_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                          const neptune_hip_apply_geom_t* g, void* x, const void* b, const void* minv, void* const work[3],
                          const void* const* in_rest, int64_t max_iters, int64_t check_every, double tol2, void* trace, void* stream,
                          const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0, double* rr_last) {
  g_pcg_rz0 = 0.0;
  return solve_checked(kSolverPcg, dtype_of_fn, stream,
                       {fn, fn_dot, body, g, x, b, minv, work, in_rest, max_iters, check_every, tol2, trace, cfg, iters_done, rr0, rr_last});
}

int neptune_hip_bicgstab_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                               const neptune_hip_apply_geom_t* g, void* x, const void* b, void* const work[5], const void* const* in_rest,
                               int64_t max_iters, int64_t check_every, double tol2, void* trace, void* stream,
                               const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0, double* rr_last) {
  return solve_checked(kSolverBicgstab, dtype_of_fn, stream,
                       {fn, fn_dot, body, g, x, b, nullptr, work, in_rest, max_iters, check_every, tol2, trace, cfg, iters_done, rr0, rr_last});
}

}  // extern "C"
