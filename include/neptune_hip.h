/*
 * neptune_hip.h -- C ABI of the MI355X (gfx950) backend for NeptuneIR's stencil hot path.
 *
 * This is the drop-in boundary.  Everything a host program (emitted host C++, the Python
 * frontend through ctypes, a PETSc MatMult thunk, the bench) needs is reachable through
 * the plain-C entry points below: plain pointers and sizes, no C++ or torch types.
 *
 * The reference project (levia-than/neptune-pde-solver) lowers `neptune_ir.apply` & co to
 * scalar CPU loop nests (lib/Passes/DataflowLowering.cpp:258-448).  The entry points here
 * are what a `backend=hip` variant of that lowering calls instead.  Each declaration cites
 * the reference construct it replaces.
 *
 * Error convention: like the reference runtime (NeptunePETScRuntime.cpp:15-30), ABI
 * functions that cannot report an error print "[NeptuneRT][HIP] ..." to stderr and abort().
 * Functions returning `int` return 0 on success and a negative NEPTUNE_HIP_E* code when the
 * request is rejected before anything is launched (bad geometry, unsupported shape).
 */
#ifndef NEPTUNE_HIP_H
#define NEPTUNE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * 1. memref descriptors of lowered functions
 *    Same field order as the reference's MLIR->LLVM memref ABI
 *    (include/Runtime/PETSc/NeptunePETScRuntime.h:22-42; rank 3 added the same way).
 *    A rank-r memref *argument* is passed expanded:
 *      (void* allocated, void* aligned, int64 offset, int64 size[0..r), int64 stride[0..r))
 *    and a memref *result* is returned as the struct by value
 *    (driver prototype: test/smoke_tests/smoke_apply.sh:39-50).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[1];
  int64_t strides[1];
} NeptuneMemRef1D;

typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[2];
  int64_t strides[2];
} NeptuneMemRef2D;

typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[3];
  int64_t strides[3];
} NeptuneMemRef3D;
/* rank 4..6 (fields with leading batch / component dimensions: the lowering peels them off and launches one rank-3
 * apply per leading index, see neptune-pde-solver_amd/csrc/runtime/lowered_runtime.hpp run_apply_batched) */
typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[4];
  int64_t strides[4];
} NeptuneMemRef4D;
typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[5];
  int64_t strides[5];
} NeptuneMemRef5D;
typedef struct {
  void *allocated;
  void *aligned;
  int64_t offset;
  int64_t sizes[6];
  int64_t strides[6];
} NeptuneMemRef6D;

/* ------------------------------------------------------------------------------------
 * 2. constants
 * ---------------------------------------------------------------------------------- */
#define NEPTUNE_HIP_MAX_RANK 3
#define NEPTUNE_HIP_MAX_INPUTS 4

#define NEPTUNE_HIP_OK 0
#define NEPTUNE_HIP_EINVAL (-1)      /* malformed geometry / null pointer            */
#define NEPTUNE_HIP_EUNSUPPORTED (-2) /* valid request this build cannot serve         */
#define NEPTUNE_HIP_EOOB (-3)        /* an access would leave its input's box (UB in the
                                        reference, DataflowLowering.cpp:382-410: no
                                        bounds check; rejected here at plan time)      */
#define NEPTUNE_HIP_ECOMM (-4)       /* RCCL / stream failure in the slab halo exchange; text in
                                        neptune_hip_slab_last_error()                   */

/* element types (the `element =` of !neptune_ir.field / !neptune_ir.temp,
 * include/Dialect/NeptuneIR/NeptuneIRTypes.td:22-33) */
#define NEPTUNE_HIP_F64 0
#define NEPTUNE_HIP_F32 1

/* kernel selection for neptune_hip_launch_cfg_t.kernel */
#define NEPTUNE_HIP_KERNEL_AUTO 0
#define NEPTUNE_HIP_KERNEL_DIRECT 1 /* one thread per cell, neighbours through L1/L2   */
#define NEPTUNE_HIP_KERNEL_MARCH 2  /* wave tiles marching along dim 0, planes in VGPRs */
/* neptune_hip_launch_cfg_t.flags */
#define NEPTUNE_HIP_FLAG_DIRECT_FLAT 1 /* direct kernel: flat one-lane-per-cell form instead of the rows form */

/* built-in stencil bodies; each one is the body of a committed fixture
 * (tests/mlir_tests/conversion_tests/) evaluated in that file's textual op order */
#define NEPTUNE_HIP_BODY_LAP2D5_F64 0  /* apply-2d-5pt.mlir   */
#define NEPTUNE_HIP_BODY_LAP3D7_F64 1  /* apply-3d-7pt.mlir   */
#define NEPTUNE_HIP_BODY_LAP3D27_F32 2 /* apply-3d-27pt.mlir  */
#define NEPTUNE_HIP_BODY_LAP1D3_F64 3  /* @ac_lap of the reference's smoke_time_advance.mlir:13-29 */
#define NEPTUNE_HIP_BODY_COUNT 4

/* ------------------------------------------------------------------------------------
 * 3. geometry of one `neptune_ir.apply`
 *    (include/Dialect/NeptuneIR/NeptuneIROps.td:164-197; semantics
 *     lib/Passes/DataflowLowering.cpp:258-448)
 *
 *    All boxes are half-open logical boxes [lb, ub) as in #neptune_ir.bounds
 *    (NeptuneIRAttrs.td:9-26).  A temp with box [lb,ub) is a dense row-major buffer of
 *    shape ub-lb (DataflowLowering.cpp:41-49); logical point p lives at physical index
 *    p - lb.  The result has box [out_lb,out_ub); input k has box [in_lb[k],in_ub[k]).
 *    shape(input 0) must equal shape(result) (cast at DataflowLowering.cpp:285-286).
 *
 *    result[q]      = input0[q]                       for every physical q   (copy-through, :283-287)
 *    result<p>      = body(p; access(k,off) = input_k<p+off>)  for p in [lb,ub)  (:289-444)
 *
 *    region: physical sub-box (result coordinates) this launch is responsible for; cells
 *    outside are not touched.  Whole field: region_lb = 0, region_ub = shape.  Used by the
 *    slab decomposition to split one apply into edge planes + interior.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  int32_t rank;       /* 1..NEPTUNE_HIP_MAX_RANK */
  int32_t num_inputs; /* 1..NEPTUNE_HIP_MAX_INPUTS */
  int64_t out_lb[NEPTUNE_HIP_MAX_RANK], out_ub[NEPTUNE_HIP_MAX_RANK];
  int64_t lb[NEPTUNE_HIP_MAX_RANK], ub[NEPTUNE_HIP_MAX_RANK]; /* apply.bounds */
  int64_t in_lb[NEPTUNE_HIP_MAX_INPUTS][NEPTUNE_HIP_MAX_RANK];
  int64_t in_ub[NEPTUNE_HIP_MAX_INPUTS][NEPTUNE_HIP_MAX_RANK];
  int64_t region_lb[NEPTUNE_HIP_MAX_RANK], region_ub[NEPTUNE_HIP_MAX_RANK];
} neptune_hip_apply_geom_t;

/* launch tuning; pass NULL (or variant = -1, kernel = chunk = 0) for the defaults */
typedef struct {
  int32_t kernel;   /* NEPTUNE_HIP_KERNEL_* */
  int32_t variant;  /* march tile variant; negative = automatic (default tile for the stencil shape);
                       see neptune_hip_march_variant_name */
  int32_t chunk;    /* march: planes per workgroup along dim 0, 0 = auto */
  int32_t flags;    /* NEPTUNE_HIP_FLAG_* bits, 0 = defaults */
} neptune_hip_launch_cfg_t;

/* ------------------------------------------------------------------------------------
 * 4. runtime: device, memory, streams
 *    The reference allocates results with malloc (memref.alloc, DataflowLowering.cpp:281)
 *    and lets the caller free() them (NeptunePETScRuntime.cpp:219-221).  Device-resident
 *    buffers follow the same callee-allocates / caller-frees rule through
 *    neptune_hip_malloc / neptune_rt_free.
 *    A lowered function stages every host-memory memref argument through a device copy; host
 *    arguments that name the identical bytes share that copy (they are one memory, as two device
 *    arguments at one address are), host arguments that overlap otherwise are refused.
 * ---------------------------------------------------------------------------------- */
/* Select the HIP device for this process (one process per GPU).  Idempotent. */
void neptune_hip_init(int device);
/* Release cached workspaces.  Safe to call more than once. */
void neptune_hip_finalize(void);
/* 1 when a HIP device is usable, 0 otherwise (never aborts). */
int neptune_hip_available(void);
/* e.g. "gfx950:sramecc+:xnack-"; pointer valid for the process lifetime */
const char *neptune_hip_arch(void);
int neptune_hip_cu_count(void);
const char *neptune_hip_version(void);

void *neptune_hip_malloc(size_t bytes);
void neptune_hip_free(void *dptr);
void neptune_hip_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
void neptune_hip_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
void neptune_hip_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
void neptune_hip_stream_sync(void *stream);
void neptune_hip_device_sync(void);
/* 1 if p is device (hipMalloc) memory, 0 if host/unknown */
int neptune_hip_is_device_ptr(const void *p);

/* ---- block pool for the temporaries of lowered functions ---------------------------------------------
 * The reference mallocs every apply result (DataflowLowering.cpp:281 -> malloc).  On the device a
 * field-sized hipMalloc/hipFree pair costs orders of magnitude more than the kernel using the block, so
 * idle blocks are cached (at most NEPTUNE_HIP_POOL_BYTES, default a quarter of the device memory) and
 * reused.  _release hands back a block that no stream still uses; a block that left a lowered function
 * as its result is simply hipFree'd by neptune_rt_free, the pool does not track live blocks. */
void *neptune_hip_pool_alloc(size_t bytes);
void neptune_hip_pool_release(void *p, size_t bytes);
void neptune_hip_pool_trim(void);
size_t neptune_hip_pool_cached_bytes(void);

/* ---- slab view for lowered modules (one process per GPU) --------------------------
 * A lowered module is compiled once, for the GLOBAL field boxes its types declare.  While a slab is
 * set, every lowered function of this process reads its memref arguments as the caller's LOCAL
 * buffers: dim 0 of every declared box [lb0,ub0) becomes [max(lb0,start-ghost_lo), min(ub0,stop+ghost_hi)),
 * apply / store / reduce bounds are clipped to the owned planes [start,stop) (logical coordinates),
 * and a reduce returns this rank's partial sum.  The caller refreshes the ghost planes of the inputs
 * (neptune_hip.slab.exchange_halos) before the call; result ghost planes are unspecified.  An apply
 * that would read ghost planes of a value produced inside the same call aborts (it needs an exchange
 * the module cannot do).  The reference has no counterpart (every PETSc object lives on
 * PETSC_COMM_SELF, NeptunePETScRuntime.cpp:136,244,257). */
int neptune_hip_set_slab(int64_t start, int64_t stop, int64_t ghost_lo, int64_t ghost_hi);
int neptune_hip_clear_slab(void);
/* out = {start, stop, ghost_lo, ghost_hi}; returns 1 if a slab is set, else 0 */
int neptune_hip_get_slab(int64_t out[4]);
/* Exchange beside interior for whole lowered functions: `event` (a hipEvent_t) marks a halo exchange of the call's
 * inputs that is still in flight on another stream.  The next lowered function then launches the interior planes of
 * its first stencil apply, makes its stream wait for the event, and launches the planes next to the ghosts; anything
 * else that comes first (a store, a reduce, a pointwise apply over the ghost planes) waits for the event before it
 * runs.  The event is consumed by that call (or by neptune_hip_clear_slab).  Needs a slab to be set. */
int neptune_hip_set_slab_pending(void *event);
void *neptune_hip_get_slab_pending(void);

/* replaces the reference's neptune_rt_free (NeptunePETScRuntime.cpp:1825 -> free()):
 * frees either a malloc'ed host result or a device result of a lowered function */
void neptune_rt_free(void *p);

/* ------------------------------------------------------------------------------------
 * 5. the hot path: apply
 * ---------------------------------------------------------------------------------- */
/* Validate a geometry against a footprint (max |offset| per input and dim): every access
 * of every in-bounds point must stay inside its input's box.  Returns NEPTUNE_HIP_OK,
 * NEPTUNE_HIP_EINVAL or NEPTUNE_HIP_EOOB.  radius[k][d] = max |offset| of input k, dim d. */
int neptune_hip_check_geom(const neptune_hip_apply_geom_t *g,
                           const int32_t radius[NEPTUNE_HIP_MAX_INPUTS][NEPTUNE_HIP_MAX_RANK]);

/* Launch one built-in body over `g` on `stream` (a hipStream_t, NULL = default stream).
 * in[k], out are DEVICE pointers to dense row-major buffers of the shapes `g` implies.
 * out must not overlap any input.  Asynchronous.
 * Replaces: the scf.for nest of ApplyToSCFForLowering (DataflowLowering.cpp:289-444)
 * plus its copy-through memref.copy (:283-287), for the body of the named fixture. */
int neptune_hip_apply_builtin(int body, const neptune_hip_apply_geom_t *g,
                              const void *const *in, void *out, void *stream,
                              const neptune_hip_launch_cfg_t *cfg);

/* A geometry-level apply entry with its body bound: what every lowered apply exports as
 * <function>_<k>__geom (csrc/lowering/emit_hip.cpp), same arguments as neptune_hip_apply_builtin
 * minus the body id. */
typedef int (*neptune_hip_apply_fn)(const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                                    void *stream, const neptune_hip_launch_cfg_t *cfg);

/* `steps` applies in a row on two ping-pong fields: step s reads fields[s % 2] as input 0 and writes
 * fields[(s + 1) % 2]; inputs 1.. (in[1..], in[0] is ignored) stay the same every step.  After the call
 * the newest state is in fields[steps % 2].  Asynchronous on `stream`.
 * The pair of launches is captured ONCE into a hipGraph and replayed (8 pairs = 16 launches per graph) (graphs are cached by
 * geometry, pointers and configuration), so the per-step host cost is a fraction of a kernel launch: for
 * fields of a few MiB -- the reference's own 1-D/2-D smoke sizes, 1024^2 -- a step is otherwise bound
 * by launch overhead, not by the kernel.  body_or_fn: pass fn = NULL to use built-in body `body`.
 * The reference's counterpart is the host loop around `entry` in a driver (smoke_apply.sh:70-80) and the
 * forward-Euler loop of its runtime (NeptunePETScRuntime.cpp:677-712). */
int neptune_hip_step_loop(neptune_hip_apply_fn fn, int body, const neptune_hip_apply_geom_t *g,
                          void *const fields[2], const void *const *in, int64_t steps, void *stream,
                          const neptune_hip_launch_cfg_t *cfg);

/* Several steps per pass over HBM.  neptune_hip_apply_chain_builtin computes out = A(A(in)) (applies = 2) or A(A(A(in)))
 * (applies = 3) for built-in body A in ONE launch -- the intermediate fields exist in registers only; the same operations on
 * the same operands as separate launches, hence the same bits.  Scope: rank 3: star footprints of input 0 up to radius 2
 * per axis (the 7-point family: two or three applies per pass; 13-point 4th-order operators: two), the fused explicit
 * Euler step of such an operator included, and -- for lowered applies -- further inputs read at the centre only
 * (coefficient fields: in[1..], the same field at every stage); rank 2: the single-input 5-point family
 * (neptune_apply_march2_rank2); when the geometry qualifies (all boxes equal, rows a whole number of 64-byte granules,
 * launch region restricted along dim 0 only); otherwise NEPTUNE_HIP_EUNSUPPORTED and nothing is launched.  neptune_hip_apply2_builtin is the
 * applies = 2 form.  Lowered applies export the same as <function>_<k>__geom2 / __geom3.
 * neptune_hip_step_loop uses them for the built-in bodies ON ITS OWN for fields of NEPTUNE_HIP_CHAIN_MIN_CELLS cells
 * (default 4e6) and more; neptune_hip_step_loop_chain is the same loop with a lowered apply's pair / triple entries `fn2`,
 * `fn3` (NULL = none) next to its single-step entry `fn` (neptune_hip_step_loop_pairs: fn3 = NULL).  The newest state ends
 * in fields[steps % 2] whatever the grouping -- and that is the ONLY field defined after the loop: with chained launches the
 * intermediate states live in registers, so fields[(steps + 1) % 2] does NOT hold state steps - 1 (with one launch per step
 * it would).  A caller that needs the previous state as well sets NEPTUNE_HIP_NO_PAIRS=1 (one launch per step) or raises
 * NEPTUNE_HIP_CHAIN_MIN_CELLS.  The reference steps one apply per pass on the host (runtime forward Euler,
 * NeptunePETScRuntime.cpp:677-712). */
int neptune_hip_apply_chain_builtin(int body, int applies, const neptune_hip_apply_geom_t *g, const void *const *in,
                                    void *out, void *stream, const neptune_hip_launch_cfg_t *cfg);
int neptune_hip_apply2_builtin(int body, const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                               void *stream, const neptune_hip_launch_cfg_t *cfg);
int neptune_hip_step_loop_pairs(neptune_hip_apply_fn fn, neptune_hip_apply_fn fn2, int body,
                                const neptune_hip_apply_geom_t *g, void *const fields[2], const void *const *in,
                                int64_t steps, void *stream, const neptune_hip_launch_cfg_t *cfg);
int neptune_hip_step_loop_chain(neptune_hip_apply_fn fn, neptune_hip_apply_fn fn2, neptune_hip_apply_fn fn3, int body,
                                const neptune_hip_apply_geom_t *g, void *const fields[2], const void *const *in,
                                int64_t steps, void *stream, const neptune_hip_launch_cfg_t *cfg);

/* Two-level (leapfrog) schemes: u(n+1) = F(u(n), u(n-1), c...), e.g. the second-order wave equation.
 * A lowered apply whose input 0 is a star of radius <= 2, whose input 1 is read at the centre only and has input 0's element
 * type, and whose further inputs are read at the centre only exports <function>_<k>__geomL2 next to __geom: ONE pair,
 *   in[0] = u(n), in[1] = u(n-1), in[2..] = centre-only inputs; out_v = u(n+1), out_w = u(n+2)
 * in one pass over HBM (csrc/kernels/apply_march2.hpp: 4.4 field passes instead of 6), bit-identical to two __geom
 * launches.  Both results are stored.  out_v and out_w must be buffers distinct from every input and from each other; the
 * geometry must qualify as for __geom2 (all boxes equal, rows a whole number of 64-byte granules, launch region
 * restricted along dim 0 only).  Anything else returns NEPTUNE_HIP_EUNSUPPORTED and nothing is launched. */
typedef int (*neptune_hip_leapfrog2_fn)(const neptune_hip_apply_geom_t *g, const void *const *in, void *out_v,
                                        void *out_w, void *stream, const neptune_hip_launch_cfg_t *cfg);

/* `steps` steps of a two-level scheme on rotating fields.  fields[0] = u(0), fields[1] = u(-1), fields[2] = scratch,
 * fields[3] = second scratch or NULL.  fn = the apply's ordinary geometry-level entry (inputs: state, previous state,
 * extra[0 .. n_extra-1]); fn2 = its leapfrog pair entry or NULL.  On return *cur / *prev are the indices into fields[]
 * that hold u(steps) and u(steps-1): BOTH are defined, whatever the grouping.  Asynchronous on `stream`.
 *   single launches: next <- F(cur, prev), then (prev, cur, next) <- (cur, next, prev): three fields, period 3;
 *   pairs (fn2 and fields[3] present): (v, w) go into the two free buffers and (prev, cur) <- (v, w): four fields, period
 *   two pair launches; an odd step count ends with one single launch.
 * Long runs replay a cached hipGraph (one linear chain of 18 single or 8 pair launches).  Whether pairs pay is measured
 * once per (entry, geometry) and process, as neptune_hip_step_loop_chain does (a pair must win by 3 %; the trial launches
 * write only into the free buffers); NEPTUNE_HIP_NO_PAIRS, NEPTUNE_HIP_TUNE=0 and NEPTUNE_HIP_CHAIN_MIN_CELLS apply
 * as there.  NEPTUNE_HIP_EUNSUPPORTED from fn2 is not an error: that (entry, geometry) runs single launches from then on. */
int neptune_hip_step_loop_leapfrog(neptune_hip_apply_fn fn, neptune_hip_leapfrog2_fn fn2,
                                   const neptune_hip_apply_geom_t *g, void *const fields[4], const void *const *extra,
                                   int n_extra, int64_t steps, void *stream, const neptune_hip_launch_cfg_t *cfg,
                                   int *cur, int *prev);
/* how many single and pair launches the last neptune_hip_step_loop_leapfrog call of this process issued or replayed
 * (its trial launches not counted) */
void neptune_hip_leapfrog_launch_counts(int64_t *singles, int64_t *pairs);

/* Systems of equations: a GROUP of sibling applies over shared inputs (2..4 members over at most 4 union inputs, e.g. the
 * (h, qx, qy) updates of a shallow-water step) that a lowered module computes in one multi-output launch exports
 * <function>_<k0>_group__geom next to its members' <function>_<k>__geom.  `g` describes the UNION inputs -- num_inputs of
 * them, in the order of the lowering report's groups[i]["inputs"] -- and the result box, apply.bounds and launch region as
 * for neptune_hip_apply_fn; out[m] is member m's result buffer.  No allocation, no synchronisation.  Every member's result
 * is always computed: in ONE launch where that form exists, else by the members' own launches (no group form for the union
 * footprint, a result not 16-byte aligned, a member's copy-through input in another box than the result,
 * NEPTUNE_HIP_NO_GROUPS=1) -- the same bits either way, members never read each other's results.  Refused, nothing
 * launched: a null pointer, or a result that overlaps an input or another result (NEPTUNE_HIP_EINVAL); a member reaching
 * outside an input's box (NEPTUNE_HIP_EOOB). */
typedef int (*neptune_hip_group_fn)(const neptune_hip_apply_geom_t *g, const void *const *in, void *const *out,
                                    void *stream, const neptune_hip_launch_cfg_t *cfg);

/* `steps` steps of a system on two SETS of fields.  Member m advances union input through[m] (the report's
 * groups[i]["through"]); fields_a[m] / fields_b[m] are that unknown's two buffers, n_out = 2..4 of them.  Step s reads set
 * s % 2 (0 = a) at the inputs through[m] and writes the other set; union inputs that are nobody's unknown (a bathymetry, a
 * coefficient field) are fixed: in[k] supplies them, the other slots of `in` are ignored (in may be NULL when there are
 * none).  After the call the newest state is in set steps % 2; every launch is one step, so the OTHER set holds state
 * steps - 1.  Asynchronous on `stream`; long runs replay a cached hipGraph (one linear chain of 16 launches), as
 * neptune_hip_step_loop does; one launch kind, no trial launches; inside a caller's stream capture plain launches.
 * NEPTUNE_HIP_EINVAL before anything runs: n_out outside 2..4, a through[] out of range or repeated, two of the 2 n_out
 * buffers equal, a fixed input missing.  steps = 0 touches nothing. */
int neptune_hip_step_loop_system(neptune_hip_group_fn fn, const neptune_hip_apply_geom_t *g, int n_out, const int *through,
                                 void *const *fields_a, void *const *fields_b, const void *const *in, int64_t steps,
                                 void *stream, const neptune_hip_launch_cfg_t *cfg);
/* the last neptune_hip_step_loop_system call of this process: steps issued or replayed, and how many hipGraphLaunch calls
 * carried them */
void neptune_hip_system_loop_counts(int64_t *launches, int64_t *graph_launches);

/* Iteration to a tolerance: the update norm out of the apply's own launch.
 * A MONITORED launch computes exactly what neptune_hip_apply_builtin computes -- the same result, bit for bit -- and
 * additionally S = sum (new - old)^2 in the field's element type T over the cells of apply.bounds that lie in the launch
 * region: `old` is input 0 at the same physical index, d = new - old is one rounding, d * d is one rounding, no FMA.
 * Cells outside apply.bounds (copy-through), clamped or predicated-off cells and cells outside the launch region
 * contribute nothing; empty bounds give +0.  Every workgroup stores one partial at its linear index (the ragged-row and
 * row-tail launches' partials follow the march launch's), a second kernel adds the partials in index order: no atomics, the
 * same bits run after run for one launch configuration (tile, chunk), rounding-level differences between configurations.
 * sum_out is a DEVICE pointer to one T, written in stream order; the call is asynchronous.  Errors as
 * neptune_hip_apply_builtin; sum_out overlapping a field is NEPTUNE_HIP_EINVAL.  Monitored forms exist for the march kernel
 * (rank 3, both rank-2 forms, rank 1) and both direct forms; a request planned onto the plane-in-LDS kernels (or one that
 * would have to grow the partials workspace inside a stream capture) returns NEPTUNE_HIP_EUNSUPPORTED with nothing
 * launched.  The several-steps-per-pass kernels, rank 4-6 and groups have no monitored form.  No first-use measuring:
 * the automatic tile or cfg's; a tile whose monitored kernel needs scratch memory is never chosen automatically.
 * The partials workspace is the process's (like neptune_hip_reduce_workspace): monitored launches on two streams at once
 * are not supported.  Lowered applies export the same as <function>_<k>__geomN on request (include/neptune_lowering.h). */
int neptune_hip_apply_builtin_norm(int body, const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                                   void *sum_out, void *stream, const neptune_hip_launch_cfg_t *cfg);
typedef int (*neptune_hip_apply_norm_fn)(const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                                         void *sum_out, void *stream, const neptune_hip_launch_cfg_t *cfg);
/* device buffer of at least `bytes` bytes for the partials of one monitored launch: grown on demand (which waits for
 * the device), released by neptune_hip_finalize; NULL when it would have to grow while `stream` is being captured */
void *neptune_hip_monitor_workspace(size_t bytes, void *stream);
/* The same S from two fields, in one read-only pass: *sum_out = sum (a - b)^2 over apply.bounds x launch region of `g`
 * (a = a field in the result's box -- the new state --, b = one in input 0's box -- the old state), the two roundings
 * above, summed by the fixed tree of the reduce(apply) kernels (another order than a monitored launch's: the two agree
 * within 2 (n - 1) eps sum |x_i|).  dtype: NEPTUNE_HIP_F64 / _F32.  sum_out: DEVICE pointer; asynchronous. */
int neptune_hip_update_norm(int dtype, const neptune_hip_apply_geom_t *g, const void *a, const void *b, void *sum_out,
                            void *stream);

/* Iterate u <- A(u) on two ping-pong fields until S = sum (A(u) - u)^2 <= tol2 or max_steps steps have run.
 * The loop runs in blocks of check_every steps (the last block shorter, so that max_steps is never exceeded): the first
 * steps of a block go through neptune_hip_step_loop_chain's loop (fn2 / fn3 = NULL: graphs as there), the LAST step of
 * every block is a monitored launch through fn_norm (fn = NULL: built-in body `body` through
 * neptune_hip_apply_builtin_norm).  After each block the scalar is read back -- one stream synchronise, sizeof(T) bytes --
 * and the loop stops when S <= tol2.  tol2 is the threshold on S itself: no square root anywhere.  A NaN sum never
 * satisfies the test, so such a loop runs to max_steps.  On return *steps_done steps have run, the newest state is in
 * fields[*steps_done % 2] and -- the last launch always being a single step -- the other field holds state
 * *steps_done - 1; *last_sum is the last S read (0 when no step ran).  steps_done / last_sum may be NULL.
 * Fallback: when fn_norm is NULL (with fn set) or the monitored entry answers NEPTUNE_HIP_EUNSUPPORTED, the checked step
 * is a plain launch followed by neptune_hip_update_norm over both fields: the same S, another summation order.
 * Synchronous by nature.  NEPTUNE_HIP_EINVAL, nothing launched: a call while `stream` is being captured, check_every < 1,
 * max_steps < 0, equal or null fields.  Element type: the built-in body's, or `dtype_of_fn` for fn (NEPTUNE_HIP_F64 /
 * NEPTUNE_HIP_F32; ignored for built-in bodies). */
int neptune_hip_step_loop_until(neptune_hip_apply_fn fn, neptune_hip_apply_norm_fn fn_norm, int body, int dtype_of_fn,
                                const neptune_hip_apply_geom_t *g, void *const fields[2], const void *const *in,
                                int64_t max_steps, int64_t check_every, double tol2, void *stream,
                                const neptune_hip_launch_cfg_t *cfg, int64_t *steps_done, double *last_sum);
/* the last neptune_hip_step_loop_until call of this process: checked steps that ran as monitored launches, checked steps
 * that ran the fallback, and checks (read-backs) in all */
void neptune_hip_until_loop_counts(int64_t *fused, int64_t *fallback, int64_t *checks);

/* Device-resident conjugate gradients: the dot products out of the launches that move the data.
 * A DOT-MONITORED launch is a monitored launch (above) with another term: D = sum new * old over the cells of apply.bounds
 * that lie in the launch region -- one rounding of the product of the fresh value and input 0 at the same physical index, in
 * the element type T; a cell that does not count adds +0.  With in[0] = p it returns q = A(p) exactly as
 * neptune_hip_apply_builtin computes it and p . A(p) out of the same launch.  Same tree, workspace, refusals
 * (NEPTUNE_HIP_EUNSUPPORTED, nothing launched: a plan onto the plane-in-LDS kernels, every tile spilling, workspace growth
 * under capture; dot_out overlapping a field: NEPTUNE_HIP_EINVAL) and asynchrony as neptune_hip_apply_builtin_norm.
 * Lowered applies export the same as <function>_<k>__geomD on request (lowering option dot-entries). */
int neptune_hip_apply_builtin_dot(int body, const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                                  void *dot_out, void *stream, const neptune_hip_launch_cfg_t *cfg);
typedef int (*neptune_hip_apply_dot_fn)(const neptune_hip_apply_geom_t *g, const void *const *in, void *out,
                                        void *dot_out, void *stream, const neptune_hip_launch_cfg_t *cfg);
/* The same D from two fields, in one read-only pass: *out_dev = sum a * b over apply.bounds x launch region of `g` (a = a
 * field in the result's box, b = one in input 0's box), summed by the fixed tree of the reduce(apply) kernels: the
 * counterpart of neptune_hip_update_norm, within 2 (n - 1) eps sum |a_i b_i| of a dot-monitored launch's D.
 * dtype: NEPTUNE_HIP_F64 / _F32.  out_dev: DEVICE pointer; asynchronous. */
int neptune_hip_dot(int dtype, const neptune_hip_apply_geom_t *g, const void *a, const void *b, void *out_dev,
                    void *stream);

/* Solve A(x) = b by unpreconditioned conjugate gradients for the apply `fn` (fn = NULL: built-in body `body`), whose
 * input 0 must have the result's box; inputs 1.. are fixed fields, in_rest[i] = input i + 1 (NULL when there is none).
 * The unknowns are the cells of Omega = apply.bounds x launch region of `g`.  x: initial guess in, solution out; cells of x
 * outside Omega keep their values (the flat update adds alpha * (+0) there) and enter only through A(x) in the initial
 * residual (Dirichlet data).  b: right-hand
 * side.  work[3] = r, p, q: caller-supplied fields of the same box; nothing but a small scalar / partials block is
 * allocated by the call.  All arithmetic in the element type T, no FMA:
 *   set-up     q = A(x);  r = b - q on Omega, +0 elsewhere;  p = r;  rr_0 = sum r * r
 *   iteration  q = A(p), pq = sum_Omega q * p out of the same launch (fn_dot);  alpha = rr / pq;
 *              x = x + (alpha p), r = r - (alpha q) on the whole flat buffers, rr' = sum r * r out of that launch;
 *              beta = rr' / rr;  p = r + (beta p);  rr <- rr'
 * An iteration that finds rr == 0 or pq == 0 uses alpha = beta = 0.  Sums: the fixed tree of the monitored launches, no
 * atomics.  alpha and beta never leave the device: the scalars live in a device block that one-workgroup kernels rotate, so
 * an iteration's launches have fixed arguments and blocks of iterations replay as hipGraphs.
 * The loop runs in blocks of check_every iterations (the last one shortened: max_iters is never exceeded); after each block
 * one stream synchronise and one sizeof(T) read, and the loop stops when rr <= tol2 (the threshold on rr itself; a NaN
 * never satisfies it).  *rr0 = rr_0 (read back once after the set-up, for a relative tolerance); rr_0 <= tol2 returns with
 * zero iterations.  *iters_done, *rr_last: iterations run, the last rr read.  trace: NULL, or a DEVICE pointer to
 * 2 * max_iters values of T: iteration k stores pq_k at [2 k] and rr_(k+1) at [2 k + 1].
 * Fallback: when fn_dot is NULL (with fn set) or answers NEPTUNE_HIP_EUNSUPPORTED (remembered for the rest of the call),
 * q = A(p) is a plain launch followed by neptune_hip_dot.
 * NEPTUNE_HIP_EINVAL, nothing launched: a call while `stream` is being captured, check_every < 1, max_iters < 0, a null
 * field, input 0's box differing from the result's, any two of x, b, r, p, q overlapping, a trace that overlaps a field. */
int neptune_hip_cg_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                         const neptune_hip_apply_geom_t *g, void *x, const void *b, void *const work[3],
                         const void *const *in_rest, int64_t max_iters, int64_t check_every, double tol2, void *trace,
                         void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double *rr0,
                         double *rr_last);
/* the last neptune_hip_cg_solve / neptune_hip_pcg_solve / neptune_hip_bicgstab_solve call of this process, whichever solver
 * ran last: iterations whose q = A(p) (BiCGStab: t = A(s)) ran as a dot-monitored launch, iterations
 * that ran the fallback, and read-backs after blocks (the read of rr_0 is not counted) */
void neptune_hip_cg_counts(int64_t *fused, int64_t *fallback, int64_t *checks);

/* The same solve with a diagonal (Jacobi) preconditioner fused into the solver's kernels.  Everything is as
 * for neptune_hip_cg_solve -- element type T, no FMA, the fixed summation tree, no atomics, Omega, the work fields, the
 * blocks of check_every iterations, the fallback, the replay schedule -- except where stated here.  minv: a device field in
 * the box of x holding M^-1; it must be finite on every cell of the box, is meant to be positive (not checked on the
 * device), and cells outside Omega should hold 1.  z = minv * r is never stored: the kernels that stream r form it in
 * registers, one rounding, from the same two operands wherever it is needed, so it has the same bits everywhere.
 *   set-up     q = A(x);  r = b - q on Omega, +0 elsewhere;  p = minv * r on Omega (one rounding), +0 elsewhere through the
 *              same select;  rz_0 = sum r * (minv * r) (two roundings per term: z = minv * r, then r * z);  rr_0 = sum r * r
 *   iteration  q = A(p), pq = sum_Omega q * p out of the same launch (fn_dot; the fallback of neptune_hip_cg_solve);
 *              alpha = rz / pq;  x = x + (alpha p), r = r - (alpha q) on the whole flat buffers, and out of that launch, from
 *              the freshly stored r, rz' = sum r * (minv * r) and rr' = sum r * r;
 *              beta = rz' / rz;  p = (minv * r) + (beta p) on the whole flat buffers;  rz <- rz', rr <- rr'
 * An iteration that finds rz == 0 or pq == 0 uses alpha = beta = 0.  The loop stops on rr <= tol2 -- the true residual,
 * exactly the meaning tol2 has in neptune_hip_cg_solve; a NaN never stops it; *rr0 and *rr_last are rr_0 and the last rr
 * read.  trace: NULL, or a DEVICE pointer to 3 * max_iters values of T: iteration k stores pq_k, rz_(k+1), rr_(k+1) at
 * [3 k], [3 k + 1], [3 k + 2].  The counters are those of neptune_hip_cg_counts.  With minv = 1 everywhere the recurrences
 * are those of neptune_hip_cg_solve (1 * r is r, rz is rr).
 * NEPTUNE_HIP_EINVAL, nothing launched: the refusals of neptune_hip_cg_solve, and a null minv, a minv that is misaligned
 * for T, a minv that overlaps any of x, b, r, p, q or the trace. */
int neptune_hip_pcg_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                          const neptune_hip_apply_geom_t *g, void *x, const void *b, const void *minv,
                          void *const work[3], const void *const *in_rest, int64_t max_iters, int64_t check_every,
                          double tol2, void *trace, void *stream, const neptune_hip_launch_cfg_t *cfg,
                          int64_t *iters_done, double *rr0, double *rr_last);
/* rz_0 = sum r * (minv * r) after the set-up of the last neptune_hip_pcg_solve call of this process (0 when it was refused):
 * with *rr0 and the trace, every scalar the recurrences used -- alpha_0 = rz_0 / pq_0 -- so that a run can be replayed */
double neptune_hip_pcg_rz0(void);

/* Solve A(x) = b by unpreconditioned BiCGStab for an apply that need not be symmetric.  Everything is as
 * for neptune_hip_cg_solve -- element type T, no FMA (one rounding per operation), A and its inputs, Omega, the fixed
 * summation tree, no atomics, the blocks of check_every iterations, the read-backs -- except where stated here.
 * work[5] = r, rh, p, v, t: caller-supplied fields of the box of x; s lives in r between the two half-steps.
 *   set-up     v = A(x) (plain launch);  r = b - v on Omega, +0 elsewhere;  rh = r;  p = r;  rr_0 = sum r * r;  rho_0 := rr_0
 *              (the same value, not a second sum).  Where the launch region is not the whole box, v and t are zeroed once
 *              before the set-up.
 *   iteration  1. v = A(p) (plain launch);  rv = sum rh * v over all n cells of the flat buffers (v is +0 outside Omega)
 *              2. alpha = rho / rv;  r = r - (alpha v) on all n cells: this is s
 *              3. t = A(s) and ts = sum_Omega t * s out of the same dot-monitored launch (fn_dot);  tt = sum t * t over all n
 *                 cells in a read-only pass over t
 *              4. omega = ts / tt;  x = (x + (alpha p)) + (omega s);  r = s - (omega t);  out of that launch, from the freshly
 *                 stored r, rho' = sum rh * r and rr' = sum r * r
 *              5. beta = (rho' / rho) * (alpha / omega): two divisions, then one product;  p = r + (beta (p - (omega v)));
 *                 rho <- rho', rr <- rr'
 * Breakdown: alpha = 0 when rho == 0 or rv == 0; omega = 0 when tt == 0; beta = 0 when rho == 0, rv == 0 or omega == 0: nothing
 * becomes NaN from finite data.  The loop stops on rr <= tol2 exactly as neptune_hip_cg_solve's (a NaN never stops it;
 * rr_0 <= tol2 returns with zero iterations).  trace: NULL, or a DEVICE pointer to 5 * max_iters values of T: iteration k
 * stores rv_k, ts_k, tt_k, rho_(k+1), rr_(k+1) at [5 k .. 5 k + 4]; with *rr0 these are every scalar the recurrences used
 * (alpha, omega, beta follow by the divisions above).  The counters are those of neptune_hip_cg_counts.
 * Fallback: when fn_dot is NULL (with fn set) or answers NEPTUNE_HIP_EUNSUPPORTED (remembered for the rest of the call),
 * step 3 is a plain launch followed by ONE flat pass over t and s that forms ts and tt (both over all n cells: s is +0
 * outside Omega).
 * NEPTUNE_HIP_EINVAL, nothing launched: the refusals of neptune_hip_cg_solve, any two of the seven fields x, b, r, rh, p, v, t
 * overlapping, a trace that overlaps a field. */
int neptune_hip_bicgstab_solve(neptune_hip_apply_fn fn, neptune_hip_apply_dot_fn fn_dot, int body, int dtype_of_fn,
                               const neptune_hip_apply_geom_t *g, void *x, const void *b, void *const work[5],
                               const void *const *in_rest, int64_t max_iters, int64_t check_every, double tol2,
                               void *trace, void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done,
                               double *rr0, double *rr_last);

/* Device-resident geometric multigrid: V-cycles over a hierarchy of applies.
 * ARITHMETIC.  Everything in the element type T (NEPTUNE_HIP_F64 / _F32), one rounding per operation, no FMA, every
 * intermediate a named temporary.  No reduction enters a field: the fields of a run are fully determined, bit for bit.
 * LEVELS.  L >= 1 levels, level 0 the finest.  Level l has a geometry g_l (rank 1..3, one rank for all levels, input 0's
 * box = the result's box), an operator A_l (fn, or fn = NULL: built-in body `body`, whose element type must be the call's)
 * with fixed inputs in_rest (in_rest[i] = input i + 1), and the fields x_l, b_l, q_l, minv_l in that box.  Omega_l =
 * apply.bounds x launch region of g_l as a physical [lo, hi) per dimension, m_l[d] = hi - lo >= 1.  The grids are
 * vertex-centred with a Dirichlet rim.  Between neighbouring levels l and l+1 every dimension d is in one of two states
 * (semi-coarsening), inferred from the extents -- for m >= 1 both cannot hold:
 *   COARSENED  m_l[d] = 2 m_(l+1)[d] + 1: the coarse cell with interior index j (counted from Omega's lower corner)
 *              coincides with the fine cell of interior index 2 j + 1;
 *   KEPT       m_l[d] = m_(l+1)[d]: the coarse cell with interior index j coincides with the fine cell of interior index j.
 * At least one dimension must be coarsened; a dimension that is neither, or a pair with none coarsened, is refused.
 * CELL-CENTRED PAIRS.  Between neighbouring levels a dimension may be in a third state, inferred from the
 * extents as the other two are -- for m >= 1 no two states can hold at once:
 *   HALVED     m_l[d] = 2 m_(l+1)[d]: the coarse cell of interior index j covers the fine cells of interior index 2 j and
 *              2 j + 1.
 * A pair of levels must have at least one dimension COARSENED or HALVED.  A pair that has both a COARSENED and a HALVED
 * dimension is refused with NEPTUNE_HIP_EINVAL and nothing is launched: one pair is one grid kind; KEPT dimensions mix
 * with either, and a hierarchy may change its grid kind from one pair to the next.  The arithmetic rules are the ones
 * above (T, one rounding per operation, no FMA, named temporaries, dimension rank-1, then rank-2, then rank-3, kept ones
 * skipped).  For a pair with halved dimensions:
 *   RESTRICTION, fused with the residual:  d = b - q on the fine Omega;  along each halved dimension  t = 0.5 * (a[2 j] +
 *     a[2 j + 1])  (one rounded addition and an exact scaling);  then  b_(l+1) = rscale_l * t  and  x_(l+1) = +0  on
 *     Omega_(l+1).  No fine cell outside Omega_l is read: there is no rim operand at all.
 *   PROLONGATION AND CORRECTION:  along a halved dimension the fine cell i takes  e[i / 2]  itself -- no operation, so -0
 *     and NaN keep their bits --, then  x_l = x_l + e  on Omega_l.  No coarse cell outside Omega_(l+1) is read.
 * The pair satisfies P = 2^k R^T for k halved dimensions, which keeps the V-cycle a symmetric preconditioner
 * (neptune_hip_mgcg_solve requires one).  Boundary conditions live entirely in the operator the caller lowers (face
 * coefficients that vanish on a Neumann face, a diagonal term for a Dirichlet face): the transfers do not know about them.
 * The pure-Neumann problem is singular and is served as it stands: the coarsest level runs sweeps, not an exact solve, the
 * right-hand side must be compatible (it must sum to zero over Omega_0), and the mean of x is whatever the iteration
 * leaves.  A level whose operator has a zero diagonal (a 1 x 1 Neumann level) cannot be smoothed: end such a hierarchy
 * at extent 2 (a non-finite minv is not refused).
 * LINEAR PROLONGATION OF A CELL-CENTRED PAIR, chosen per pair by the caller
 * (neptune_hip_mg_prolong_t below; the default stays the piecewise-constant one above).  The arithmetic rules are the ones
 * above: T, one rounding per operation, no FMA, named temporaries, dimension rank-1, then rank-2, then rank-3, kept ones
 * skipped.  Along one halved dimension let e[0 .. m_c) be the coarse values -- the values AFTER the dimensions already
 * done.  A fine cell of interior index i has j = i / 2, and its neighbour is n = j - 1 for even i, n = j + 1 for odd i:
 *     v = e[n]                   if 0 <= n < m_c
 *     v = +e[j]   (rule EVEN)    if n is outside: a Neumann face, the ghost cell mirrored
 *     v = -e[j]   (rule ODD)     if n is outside: the value 0 ON the face, the ghost cell mirrored with its sign flipped
 *     p = 0.75 * e[j];   s = 0.25 * v;   t = p + s
 *   then  x_l = x_l + t  on Omega_l.  The rule is given per face, low and high, per dimension.  In the tensor product the
 *   ghost of a later dimension is +- the INTERMEDIATE at the edge (what padding the intermediate array gives).  m_c = 1
 *   makes both neighbours ghosts.  No coarse cell outside Omega_(l+1) is read, no fine cell outside Omega_l is written;
 *   along a kept dimension the transfer is the identity.  With the averaging restriction P != c R^T and the cycle is NOT a
 *   symmetric preconditioner: the neptune_hip_mgcg_* entries take such a pair only with the restriction below.
 * TRANSPOSED LINEAR RESTRICTION OF A CELL-CENTRED PAIR, chosen per pair by the caller
 * (neptune_hip_mg_transfer_t below; the default stays the averaging one above): R = P^T / 2^k for k halved dimensions, P the
 * linear prolongation above BY THE SAME RULE PER FACE.  The arithmetic rules are the ones above: T, one rounding per
 * operation, no FMA, named temporaries, dimension rank-1, then rank-2, then rank-3, kept ones the identity.  Fused with the
 * residual as the other restrictions:  d = b - q on the fine Omega.  Along one halved dimension let a[0 .. 2 m_c) be the
 * values AFTER the dimensions already done.  For the coarse index j:
 *     a_m = a[2 j - 1]   if j >= 1,          else  +a[0] (rule_lo EVEN)  or  -a[0] (rule_lo ODD)
 *     a_p = a[2 j + 2]   if j <= m_c - 2,    else  +a[2 m_c - 1] (rule_hi EVEN)  or  -a[2 m_c - 1] (rule_hi ODD)
 *     s_m = 0.25 * a_m;   p_0 = 0.75 * a[2 j];   p_1 = 0.75 * a[2 j + 1];   s_p = 0.25 * a_p
 *     u = s_m + p_0;   v = p_1 + s_p;   w = u + v;   t = 0.5 * w
 *   then  b_(l+1) = rscale_l * t  and  x_(l+1) = +0  on Omega_(l+1).  The ghost is an exact sign flip.  In the tensor
 *   product a later dimension's ghost is +- the INTERMEDIATE at the edge: padding the fine array with +- its edge is exactly
 *   the transpose of padding the coarse array with +- its edge.  m_c = 1 makes both outer operands ghosts.  No fine cell
 *   outside Omega_l is read, no coarse cell outside Omega_(l+1) is written.  In exact arithmetic this is P^T / 2 per halved
 *   dimension: interior weights 1/8, 3/8, 3/8, 1/8; end weights 1/2, 3/8, 1/8 under EVEN and 1/4, 3/8, 1/8 under ODD.  With
 *   the LINEAR prolongation the pair satisfies P = 2^k R^T and the V-cycle is a symmetric preconditioner again.
 * Along a kept dimension both transfers are the identity -- no operation, no rounding, -0 and NaN keep their bits: the
 * restriction hands d = b - q through to the next dimension, the prolongation takes e[j] itself, and there is no rim
 * along it.  The coarsened dimensions run in the order stated below, the kept ones skipped.  With every dimension
 * coarsened this is full coarsening.
 * SMOOTHING SWEEP on level l (damped Jacobi; the caller folds omega / diagonal into minv):  q = A_l(x) as a plain launch of
 * g_l, then on Omega_l only  d = b - q,  w = minv * d,  x = x + w.  Cells of x outside Omega_l are not written; minv outside
 * Omega_l is never read.
 * RESTRICTION l -> l+1, fused with the residual (r is never a field):  d<f> = b_l<f> - q_l<f> (q_l = A_l(x_l) from a plain
 * launch just before), then the one-dimensional stencil  t = ((0.25 a-) + (0.5 a0)) + (0.25 a+)  centred on fine interior
 * index 2 j + 1, along dimension rank-1 (the contiguous one) first, then rank-2, then rank-3 (kept dimensions skipped); then
 * b_(l+1)<c> = rscale_l * t  and  x_(l+1)<c> = +0  for every c in Omega_(l+1).  Cells outside Omega_(l+1) are not written,
 * and no fine cell outside Omega_l is read.
 * PROLONGATION AND CORRECTION l+1 -> l.  Along one axis a fine cell of interior index i takes  e[(i - 1) / 2]  for odd i and
 * 0.5 * (e[i / 2 - 1] + e[i / 2])  for even i (one rounded addition, then the exact scaling), with e[-1] = e[m_(l+1)] = +0
 * whatever the coarse field holds outside Omega_(l+1).  The tensor product runs along dimension rank-1 first, then rank-2,
 * then rank-3 (kept dimensions skipped: the coarse rim is +0 along coarsened dimensions only); then  x_l = x_l + e  on
 * Omega_l.  Cells outside keep their bits.
 * CYCLE(l).  On level L-1: coarse_sweeps smoothing sweeps.  On any other level: `pre` sweeps;  q = A(x) and the
 * restriction;  Cycle(l+1);  prolongation and correction;  `post` sweeps.
 * The three kernels alone (asynchronous on `stream`; NEPTUNE_HIP_EINVAL, nothing launched: a null pointer, an unknown
 * dtype, a malformed geometry, an empty Omega, ranks that differ, the size relation violated (a dimension neither
 * coarsened, halved nor kept, none coarsened or halved, or a coarsened and a halved one in the same pair), a non-finite
 * rscale, a written field overlapping a field the same launch reads).  neptune_hip_mg_restrict and _prolong_add dispatch on
 * the pair's inferred grid kind: */
int neptune_hip_mg_smooth(int dtype, const neptune_hip_apply_geom_t *g, const void *q, const void *b, const void *minv,
                          void *x, void *stream);
int neptune_hip_mg_restrict(int dtype, const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                            const void *b_fine, const void *q_fine, double rscale, void *b_coarse, void *x_coarse,
                            void *stream);
int neptune_hip_mg_prolong_add(int dtype, const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                               const void *x_coarse, void *x_fine, void *stream);
/* What a pair of levels means: *mask_out = the dimensions coarsened or halved between g_fine and g_coarse (the union of
 * the COARSENED and the HALVED ones), bit d = field dimension d (the others are kept).  Host-side geometry only, nothing is
 * launched.  NEPTUNE_HIP_EINVAL, *mask_out untouched, where the transfers would refuse the pair: a null pointer, a
 * malformed geometry, an empty Omega, ranks that differ, a dimension in none of the three states, no dimension coarsened
 * or halved, a coarsened and a halved dimension in the same pair. */
int neptune_hip_mg_coarsened_axes(const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                                  int *mask_out);
/* *mask_out = the HALVED dimensions only: 0 for a vertex-centred pair, the mask of neptune_hip_mg_coarsened_axes for a
 * cell-centred one.  It refuses the same pairs as neptune_hip_mg_coarsened_axes. */
int neptune_hip_mg_halved_axes(const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                               int *mask_out);
/* One level of a hierarchy.  Level 0's x and b are the caller's problem: initial guess in, solution out, and the
 * right-hand side; the cells of x_0 outside Omega_0 are Dirichlet data that enter through A(x) only.  x_l, b_l of the
 * coarser levels and every q_l are work fields: what they hold on entry does not matter. */
typedef struct {
  neptune_hip_apply_fn fn; int body;          /* fn = NULL: built-in body */
  neptune_hip_apply_geom_t g;
  const void *const *in_rest;                 /* inputs 1.., NULL when none */
  const void *minv;  void *x, *b, *q;         /* level 0: x and b are the caller's */
  double rscale;                              /* applied by the restriction that LEAVES this level; unused on the last */
} neptune_hip_mg_level_t;
/* SOLVE.  x_l for l >= 1 is zero-filled once, whole box.  rr_0 = sum over Omega_0 of (b - A(x))^2: a plain launch into q_0,
 * then neptune_hip_update_norm.  rr_0 <= tol2 returns with zero cycles.  Otherwise blocks of check_every cycles (the last
 * one shortened: max_cycles is never exceeded); after each block the same rr, one stream synchronise and one scalar read;
 * the loop stops on rr <= tol2 (the threshold on rr itself; a NaN never stops it).  Every rr read after a block is also
 * stored into rr_checks, a HOST array of ceil(max_cycles / check_every) doubles, or NULL.  *cycles_done, *rr0, *rr_last
 * (each may be NULL): cycles run, rr_0, the last rr read.  cfg: the launch configuration of level 0's operator; the
 * coarser levels launch with the defaults.
 * REPLAY.  The first cycle of a call runs as plain launches.  When at least two more cycles may follow, one cycle is
 * captured once on the call's stream -- a linear graph, no parallel branches -- and every further cycle is one
 * hipGraphLaunch of it; the graph is destroyed when the call returns.  A launch that refuses under capture ends the capture,
 * the graph is discarded and the call goes on with plain launches: not an error.  Environment NEPTUNE_HIP_MG_GRAPH=0
 * (read at every call) disables the graph path.
 * NEPTUNE_HIP_EINVAL, nothing launched: n_levels < 1 or > 16, a rank that differs between levels, the size relation
 * violated in any dimension, an empty Omega, a null field, a missing fixed input, any two of a level's x, b, q, minv
 * overlapping, a level's fields overlapping those of a neighbouring level, input 0's box differing from the result's,
 * negative pre, post or coarse_sweeps, check_every < 1, max_cycles < 0, a stream that is being captured, a non-finite
 * rscale on a level that has a coarser one, an unknown dtype, a built-in body of another element type. */
int neptune_hip_mg_solve(const neptune_hip_mg_level_t *levels, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                         int64_t max_cycles, int64_t check_every, double tol2, double *rr_checks, void *stream,
                         const neptune_hip_launch_cfg_t *cfg, int64_t *cycles_done, double *rr0, double *rr_last);
/* the last neptune_hip_mg_solve call of this process: cycles that ran as plain launches, cycles that ran as graph launches,
 * and read-backs after blocks (the read of rr_0 is not counted) */
void neptune_hip_mg_counts(int64_t *plain_cycles, int64_t *graph_cycles, int64_t *checks);

/* Line smoothers: tridiagonal solves along any axis in place of the point sweep.
 * ARITHMETIC as above: element type T, one rounding per operation, no FMA, every intermediate a named temporary, no
 * reduction enters a field: every field of a run stays determined bit for bit.
 * A LINE STAGE on level l is a field dimension a, 0 <= a < rank, plus three factor fields lo, inv, up in the level's box.
 * It runs  q = A_l(x)  as a plain launch, then for every line of Omega_l along a -- the other interior indices fixed,
 * m = m_l[a], interior index i --
 *   forward    d_i = b_i - q_i;   g_0 = d_0 * inv_0;   for i >= 1:  t = lo_i * g_(i-1),  s = d_i - t,  g_i = s * inv_i
 *   backward   e_(m-1) = g_(m-1);   for i < m-1:  t = up_i * e_(i+1),  e_i = g_i - t
 *   update     x_i = x_i + e_i
 * lo_0, up_(m-1) and the factor fields outside Omega are never read.  x outside Omega keeps its bits.  q on Omega holds
 * unspecified values afterwards (the kernel keeps g there: q is not const); outside Omega q keeps its bits.  m = 1 is
 * x = x + inv * (b - q): the point sweep's bits when inv = minv.  The values are those of these recurrences, so the solve
 * along a line is sequential.
 * THE FACTORS are Thomas's elimination of T / omega, T the tridiagonal part (l_i, t_i, u_i) of A_l along a restricted to
 * Omega -- couplings to rim cells are dropped: they are Dirichlet data.  Set-up work of the caller, in T with one rounding
 * per operation:
 *   l'_i = l_i / omega,  t'_i = t_i / omega,  u'_i = u_i / omega;
 *   inv_0 = 1 / t'_0,  c_0 = u'_0 * inv_0;   for i >= 1:  p = l'_i * c_(i-1),  den = t'_i - p,  inv_i = 1 / den,  c_i = u'_i * inv_i;
 *   lo = l',  up = c;  all three +0 outside Omega, lo +0 at i = 0 and up +0 at i = m-1.
 * A SWEEP on a level that has k >= 1 stages runs all k, each with its own apply.  Pre-sweeps and the last level's coarse
 * sweeps run stages 0 .. k-1, post-sweeps run k-1 .. 0: a cycle with symmetric stages stays symmetric.  A level with k = 0
 * runs the point sweep with minv.
 * The stage's kernel alone (asynchronous on `stream`): the refusals of neptune_hip_mg_smooth, and NEPTUNE_HIP_EINVAL,
 * nothing launched, for an axis outside the rank, a null factor field, x or q overlapping any other field of the call. */
int neptune_hip_mg_line_smooth(int dtype, const neptune_hip_apply_geom_t *g, int axis, void *q, const void *b, const void *lo,
                               const void *inv, const void *up, void *x, void *stream);
/* The stages of one level: stage s runs along field dimension axis[s] with the factor fields lo[s], inv[s], up[s]. */
typedef struct { int32_t n_stages; int32_t axis[3]; const void *lo[3], *inv[3], *up[3]; } neptune_hip_mg_lines_t;
/* neptune_hip_mg_solve with line stages: lines[l] belongs to levels[l]; the solve, the stop rule, rr_checks, the replay (a
 * stage is two plain launches: the captured cycle stays a linear graph) and the counts are neptune_hip_mg_solve's.
 * lines == NULL, or n_stages = 0 on every level, is neptune_hip_mg_solve exactly -- the same launches, the same bits --
 * and neptune_hip_mg_solve is that call.  A level with stages does not read minv, which may then be NULL.
 * NEPTUNE_HIP_EINVAL, nothing launched: the refusals of neptune_hip_mg_solve, n_stages outside 0..3, an axis outside the
 * rank, a null or misaligned factor field, a factor field overlapping the level's x, b, q or those of a neighbouring
 * level.  neptune_hip_mgcg_solve itself takes no lines (its fused first and last sweeps on level 0 are point Jacobi);
 * neptune_hip_mgcg_solve_lines below does. */
int neptune_hip_mg_solve_lines(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, int n_levels,
                               int dtype, int pre, int post, int coarse_sweeps, int64_t max_cycles, int64_t check_every,
                               double tol2, double *rr_checks, void *stream, const neptune_hip_launch_cfg_t *cfg,
                               int64_t *cycles_done, double *rr0, double *rr_last);

/* The prolongation of one pair of levels: the piecewise-constant / interpolating one the pair's grid kind
 * implies (CONSTANT: what neptune_hip_mg_prolong_add does), or the LINEAR one of a cell-centred pair defined above, with a
 * rule per face, indexed by field dimension.  Entries of dimensions >= rank, and every rule of a CONSTANT pair, are not
 * read. */
#define NEPTUNE_HIP_MG_PROLONG_CONSTANT 0
#define NEPTUNE_HIP_MG_PROLONG_LINEAR   1
#define NEPTUNE_HIP_MG_RIM_EVEN 0   /* a Neumann face: the ghost is +e at the edge */
#define NEPTUNE_HIP_MG_RIM_ODD  1   /* the value 0 on the face: the ghost is -e at the edge */
typedef struct { int32_t kind; int32_t rim_lo[3], rim_hi[3]; } neptune_hip_mg_prolong_t;   /* indexed by field dimension */
/* The prolongation kernel alone, by *p (asynchronous on `stream`): kind CONSTANT is neptune_hip_mg_prolong_add.  The
 * refusals of neptune_hip_mg_prolong_add, and NEPTUNE_HIP_EINVAL, nothing launched, for p = NULL, a kind outside {0, 1},
 * LINEAR on a pair with no halved dimension, a rule outside {0, 1} on a dimension < rank of a LINEAR pair. */
int neptune_hip_mg_prolong_add_linear(int dtype, const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                                      const neptune_hip_mg_prolong_t *p, const void *x_coarse, void *x_fine, void *stream);
/* neptune_hip_mg_solve_lines with the prolongation chosen per pair: prolong[l] belongs to the pair (l, l + 1), n_levels - 1
 * entries are read.  prolong == NULL, or kind CONSTANT everywhere, is neptune_hip_mg_solve_lines exactly -- the same
 * launches, the same bits -- and neptune_hip_mg_solve_lines is that call.  The solve, the stop rule, rr_checks, the replay
 * and the counts are neptune_hip_mg_solve's.  NEPTUNE_HIP_EINVAL, nothing launched, every field's bits unchanged: the
 * refusals of neptune_hip_mg_solve_lines and those of neptune_hip_mg_prolong_add_linear for any pair.  The
 * neptune_hip_mgcg_* entries take no such array: with a LINEAR pair the cycle is not a symmetric preconditioner. */
int neptune_hip_mg_solve_prolong(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines,
                                 const neptune_hip_mg_prolong_t *prolong, int n_levels, int dtype, int pre, int post,
                                 int coarse_sweeps, int64_t max_cycles, int64_t check_every, double tol2, double *rr_checks,
                                 void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *cycles_done, double *rr0,
                                 double *rr_last);
/* Both transfers of one pair of levels: `prolong` as neptune_hip_mg_prolong_t's kind, restrict_kind the
 * restriction, and ONE rule array for both -- a pair that restricts by one rule and prolongs by another cannot be expressed.
 * The rules are read when either transfer is LINEAR; entries of dimensions >= rank never. */
#define NEPTUNE_HIP_MG_RESTRICT_AVERAGE 0   /* what neptune_hip_mg_restrict does for the pair's grid kind */
#define NEPTUNE_HIP_MG_RESTRICT_LINEAR  1   /* the transpose of the LINEAR prolongation, by the same face rules */
typedef struct { int32_t prolong, restrict_kind; int32_t rim_lo[3], rim_hi[3]; } neptune_hip_mg_transfer_t;
/* The restriction kernel alone, by *t (asynchronous on `stream`): restrict_kind AVERAGE is neptune_hip_mg_restrict exactly;
 * t->prolong is validated and otherwise unused.  The refusals of neptune_hip_mg_restrict, and NEPTUNE_HIP_EINVAL, nothing
 * launched, for t = NULL, a prolong or restrict_kind outside {0, 1}, a LINEAR transfer on a pair with no halved dimension, a
 * rule outside {0, 1} on a dimension < rank when either transfer is LINEAR. */
int neptune_hip_mg_restrict_linear(int dtype, const neptune_hip_apply_geom_t *g_fine, const neptune_hip_apply_geom_t *g_coarse,
                                   const neptune_hip_mg_transfer_t *t, const void *b_fine, const void *q_fine, double rscale,
                                   void *b_coarse, void *x_coarse, void *stream);
/* neptune_hip_mg_solve_lines with both transfers chosen per pair: transfer[l] belongs to the pair (l, l + 1), n_levels - 1
 * entries are read; any combination is accepted per pair.  transfer == NULL, or CONSTANT / AVERAGE everywhere, is
 * neptune_hip_mg_solve_lines exactly -- the same launches, the same bits; neptune_hip_mg_solve_prolong is this call with
 * AVERAGE everywhere.  NEPTUNE_HIP_EINVAL, nothing launched, every field's bits unchanged: the refusals of
 * neptune_hip_mg_solve_lines and those of neptune_hip_mg_restrict_linear for any pair. */
int neptune_hip_mg_solve_transfer(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines,
                                  const neptune_hip_mg_transfer_t *transfer, int n_levels, int dtype, int pre, int post,
                                  int coarse_sweeps, int64_t max_cycles, int64_t check_every, double tol2, double *rr_checks,
                                  void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *cycles_done, double *rr0,
                                  double *rr_last);

/* TWO MORE FORMS OF THE STAGE'S KERNEL, alone (asynchronous on `stream`).  ARITHMETIC as above.
 * neptune_hip_mg_line_first is the APPLY-FREE stage: the values of the plain stage run on q = +0, x = +0 --
 *   d_i = b_i, the forward and backward recurrences unchanged, x_i = (+0) + e_i
 * -- the addition of +0 stays: the bits are the plain stage's, a -0 becomes +0.  It reads b, lo, inv, up and writes x on Omega
 * only; it does not read x (it keeps g there between its two marches) and has no q.  The refusals of
 * neptune_hip_mg_line_smooth, without those for q. */
int neptune_hip_mg_line_first(int dtype, const neptune_hip_apply_geom_t *g, int axis, const void *b, const void *lo,
                              const void *inv, const void *up, void *x, void *stream);
/* neptune_hip_mg_line_smooth_dot is neptune_hip_mg_line_smooth (the same update of x on Omega, the same cells read and
 * written) and *dot_out = sum over Omega of b * x_new: in the backward march t_i = b_i * x_new,i, one rounding, from the
 * freshly formed x_new; a lane adds its line's terms to one accumulator in the order of that march (i = m-1 .. 0) from +0;
 * one partial per workgroup on the fixed tree of the monitored launches (a 64-lane workgroup's partial is its single wave's
 * sum), added in index order by one workgroup.  Which lines share a workgroup is the launch's choice (the lanes of a slow-axis
 * workgroup own consecutive cells of the contiguous axis, 256 or 64 of them; a contiguous-axis workgroup owns 64 consecutive
 * lines): the sum is one of the orders this allows, and is the same from run to run.  dot_out: a DEVICE pointer to one T.
 * The refusals of neptune_hip_mg_line_smooth, and as for neptune_hip_mg_smooth_dot: NEPTUNE_HIP_EINVAL for a null or
 * misaligned dot_out or one that overlaps a field, NEPTUNE_HIP_EUNSUPPORTED, nothing launched, when `stream` is being
 * captured and the partials' workspace would have to grow. */
int neptune_hip_mg_line_smooth_dot(int dtype, const neptune_hip_apply_geom_t *g, int axis, void *q, const void *b,
                                   const void *lo, const void *inv, const void *up, void *x, void *dot_out, void *stream);

/* Multigrid-preconditioned conjugate gradients: CG on level 0 whose preconditioner is one V-cycle.
 * ARITHMETIC as above and as for neptune_hip_pcg_solve: element type T, one rounding per operation, no FMA, every
 * intermediate a named temporary, sums on the fixed tree of the monitored launches, no atomics.
 * THE SMOOTHING SWEEP WITH A SUM, alone:  neptune_hip_mg_smooth_dot is neptune_hip_mg_smooth (the same update of x on Omega,
 * the same cells read and written) and *dot_out = sum over Omega of b * x_new, one rounding per term from the b and the
 * freshly stored x of the cell, each lane's accumulator being that one term; one partial per workgroup, added in index order
 * by one workgroup.  dot_out: a DEVICE pointer to one T; asynchronous.  The refusals of neptune_hip_mg_smooth, and
 * NEPTUNE_HIP_EINVAL for a null dot_out or one that overlaps a field; NEPTUNE_HIP_EUNSUPPORTED, nothing launched, when
 * `stream` is being captured and the partials' workspace would have to grow. */
int neptune_hip_mg_smooth_dot(int dtype, const neptune_hip_apply_geom_t *g, const void *q, const void *b, const void *minv,
                              void *x, void *dot_out, void *stream);
/* SOLVE A_0(x) = b.  levels: the hierarchy of neptune_hip_mg_solve, 2 <= n_levels <= 16; level 0's x and b are the caller's
 * unknown and right-hand side, level 0's q serves both A(p) and the cycle.  work[3] = r, p, z: caller-supplied fields of
 * level 0's box.  sweeps >= 1 is the pre-sweep AND the post-sweep count of every level but the last, which runs
 * coarse_sweeps: the preconditioner is then symmetric.  A_0 is taken to be linear in input 0 (A(0) = 0), as CG assumes
 * anyway.  fn_dot: level 0's dot-monitored entry, or NULL.
 * THE PRECONDITIONER z = M(r): one V(sweeps, sweeps) cycle as defined above on A_0 z = r from z = 0, level 0's (x, b) replaced
 * by (z, r), with two differences, both on level 0:
 *   - its first pre-sweep runs no apply and is not a launch of its own: from z = 0 and A(0) = 0 it is z = minv_0 * r, one
 *     rounding, formed on EVERY cell of the flat buffer by the kernel that stores the new r.  r is +0 outside Omega_0, and
 *     minv_0 must be finite on the whole box (jacobi_weights puts +0 there; not checked on the device): z outside Omega_0 is
 *     then a zero, the zero Dirichlet rim of the error equation.
 *   - its last post-sweep is neptune_hip_mg_smooth_dot's kernel: it also yields r . z = sum over Omega_0 of r * z_new.
 * "The rest of M" below is everything after that first pre-sweep.  Levels >= 1 run exactly Cycle(l).
 *   set-up     x_l for l >= 1 is zero-filled once, whole box; where level 0's launch region is not its whole box, q_0 is
 *              zero-filled once as well (the flat update reads it everywhere).
 *              1. q = A(x), a plain launch   2. on Omega: r = b - q, z = minv_0 * r; outside: +0 for both through one select;
 *              out of that launch rr_0 = sum r * r   3. rr_0 is read back (the set-up's one synchronise): rr_0 <= tol2 or
 *              max_iters == 0 returns with zero iterations   4. the rest of M, which yields rz_0   5. p = z, a device copy of
 *              the whole box
 *   iteration  1. q = A(p) and pq = sum_Omega q * p out of one dot-monitored launch (fn_dot, or
 *                 neptune_hip_apply_builtin_dot for a built-in body)
 *              2. alpha = rz / pq;  on all cells x = x + (alpha p), r = r - (alpha q), z = minv_0 * r from the new r; out of
 *                 that launch rr' = sum r * r
 *              3. the rest of M, which yields rz'
 *              4. beta = rz' / rz;  on all cells p = z + (beta p);  rz <- rz', rr <- rr'
 * An iteration that finds rz == 0 or pq == 0 uses alpha = beta = 0.  The loop stops on rr <= tol2 exactly as
 * neptune_hip_pcg_solve's: blocks of check_every iterations (the last one shortened), after each block one stream
 * synchronise and one scalar read; a NaN never stops it.  *iters_done, *rr0, *rr_last (each may be NULL): iterations run,
 * rr_0, the last rr read.  trace: NULL, or a DEVICE pointer to 3 * max_iters values of T: iteration k stores pq_k,
 * rz_(k+1), rr_(k+1) at [3 k .. 3 k + 2].  The scalars live in a device block that one-workgroup kernels rotate, so every
 * launch of an iteration has fixed arguments.
 * Fallback: when fn_dot is NULL (with level 0's fn set) or the dot-monitored entry answers NEPTUNE_HIP_EUNSUPPORTED
 * (remembered for the rest of the call), step 1 is a plain launch followed by neptune_hip_dot.
 * REPLAY as neptune_hip_mg_solve's, per iteration: the first iteration runs as plain launches; when at least two more may
 * follow, ONE iteration is captured once as a linear graph and every later iteration is one hipGraphLaunch of it; a launch
 * that refuses under capture ends the capture and the call goes on with plain launches; NEPTUNE_HIP_MG_GRAPH=0 disables
 * the graph path.  cfg: the launch configuration of level 0's operator.
 * NEPTUNE_HIP_EINVAL, nothing launched: every refusal of neptune_hip_mg_solve that applies (pre / post read as sweeps,
 * max_cycles as max_iters), n_levels < 2, sweeps < 1, a null work array, a null or misaligned work[i] or trace, any overlap
 * among x, b, r, p, z, level 0's q and minv, the trace, and level 1's x, b, q, minv, a stream that is being captured. */
int neptune_hip_mgcg_solve(const neptune_hip_mg_level_t *levels, int n_levels, int dtype, neptune_hip_apply_dot_fn fn_dot,
                           int sweeps, int coarse_sweeps, void *const work[3], int64_t max_iters, int64_t check_every,
                           double tol2, void *trace, void *stream, const neptune_hip_launch_cfg_t *cfg,
                           int64_t *iters_done, double *rr0, double *rr_last);
/* neptune_hip_mgcg_solve WITH LINE STAGES: lines[l] belongs to levels[l] as in neptune_hip_mg_solve_lines.
 * lines == NULL, or n_stages = 0 on every level, is neptune_hip_mgcg_solve exactly -- the same launches, the same bits --
 * and neptune_hip_mgcg_solve is that call.  A level with stages does not read minv, which may then be NULL; that includes
 * level 0.  Stages on levels >= 1 change nothing else: those levels run Cycle(l) with their stages.
 * WHEN LEVEL 0 HAS k >= 1 STAGES the preconditioner z = M(r) is one V(sweeps, sweeps) cycle of neptune_hip_mg_solve_lines on
 * A_0 z = r from z = 0, with two differences, both on level 0:
 *   - the first stage (stage 0) of the first pre-sweep runs no apply: it is neptune_hip_mg_line_first's kernel on b = r,
 *     x = z.  Stages 1 .. k-1 of that sweep are plain (apply + stage).  z outside Omega_0 is zero-filled once at set-up, whole
 *     box -- the error equation's Dirichlet rim -- and nothing writes there again.
 *   - the last stage (stage 0) of the last post-sweep is neptune_hip_mg_line_smooth_dot's kernel after its own apply: it
 *     also yields r . z.
 * The set-up and the iteration are neptune_hip_mgcg_solve's step for step, except that the set-up's step 2 and the
 * iteration's step 2 store r (and x) only -- z = minv_0 * r is not formed, rr is unchanged -- and that "the rest of M"
 * starts with the apply-free stage.  Scalars, trace, stop rule, the fallback of step 1, the counts and the replay (a stage is
 * plain launches: the captured iteration stays a linear graph) are unchanged.
 * NEPTUNE_HIP_EINVAL, nothing launched: the refusals of neptune_hip_mgcg_solve, those neptune_hip_mg_solve_lines adds for
 * `lines`, and a factor field that overlaps work[0..2] or the trace. */
int neptune_hip_mgcg_solve_lines(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, int n_levels,
                                 int dtype, neptune_hip_apply_dot_fn fn_dot, int sweeps, int coarse_sweeps,
                                 void *const work[3], int64_t max_iters, int64_t check_every, double tol2, void *trace,
                                 void *stream, const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double *rr0,
                                 double *rr_last);
/* neptune_hip_mgcg_solve_lines with the transfers chosen per pair: transfer as in
 * neptune_hip_mg_solve_transfer, but a pair is accepted only if it is SYMMETRIC -- CONSTANT with AVERAGE, or LINEAR with
 * LINEAR --, so that the cycle stays a symmetric preconditioner; both level-0 seams of the iteration (the restriction and
 * the prolongation of "the rest of M") follow pair 0's choice.  transfer == NULL, or CONSTANT / AVERAGE everywhere, is
 * neptune_hip_mgcg_solve_lines exactly -- the same launches, the same bits -- and neptune_hip_mgcg_solve_lines is this call
 * with NULL.  NEPTUNE_HIP_EINVAL, nothing launched, every field's bits unchanged: the refusals of
 * neptune_hip_mgcg_solve_lines, those of neptune_hip_mg_restrict_linear for any pair, and an asymmetric pair. */
int neptune_hip_mgcg_solve_transfer(const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines,
                                    const neptune_hip_mg_transfer_t *transfer, int n_levels, int dtype,
                                    neptune_hip_apply_dot_fn fn_dot, int sweeps, int coarse_sweeps, void *const work[3],
                                    int64_t max_iters, int64_t check_every, double tol2, void *trace, void *stream,
                                    const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double *rr0, double *rr_last);
/* MIXED PRECISION: conjugate gradients in D = f64 around the preconditioner's V-cycle in S = f32.  Only
 * (dtype_outer, dtype_inner) = (NEPTUNE_HIP_F64, NEPTUNE_HIP_F32) is accepted.  Arithmetic as everywhere: one rounding per
 * operation, no FMA, every intermediate a named temporary, sums on the fixed tree of the monitored launches, no atomics;
 * operations on D values round in D, operations on S values round in S.  The two conversions:
 *   narrow(v)  D -> S, one rounding to nearest even, as the cast (float) gives it: a finite value beyond f32's range becomes
 *              +-inf, a result in f32's subnormal range is kept (the kernels run in the default mode, which preserves f32
 *              subnormals), -0 and NaN pass through
 *   widen(v)   S -> D, exact
 * No scaling of r is applied: A CALLER WHOSE RESIDUAL LEAVES f32'S RANGE (about 1e-45 .. 3e38 in magnitude) MUST SCALE THE
 * SYSTEM -- components that narrow to +-inf poison the cycle, components that narrow to 0 are not preconditioned.
 * outer: ONE level in D that carries the operator (fn / body, g, in_rest), x (the unknown), b (the right-hand side) and q; its
 * minv and rscale are not read.  fn_dot: the outer operator's dot-monitored entry, or NULL.  levels[0 .. n_levels), lines:
 * exactly a hierarchy of neptune_hip_mg_solve_lines in S, n_levels >= 2; level 0 has its own f32 operator (the same operator
 * lowered at f32, or an f32 built-in body); level 0's b is the narrowed residual r32 and level 0's x is z32, both
 * caller-supplied work fields.  levels[0].g must describe the same box and the same Omega as outer->g.  work[2] = r, p in D,
 * in level 0's box.
 * THE PRECONDITIONER z32 = M32(r32) is the preconditioner of neptune_hip_mgcg_solve word for word, run in S on (z32, r32):
 * its first pre-sweep is z32 = minv_0 * r32 on every cell, formed by the kernel that stores the residual; its last post-sweep
 * is neptune_hip_mg_smooth_dot_wide's kernel and yields r . z = sum over Omega_0 of widen(r32) * widen(z32_new) -- each
 * term exact in D, partials and root in D.  So rz = r32 . M32(r32): positive for a symmetric positive definite M32 whatever
 * the narrowing did, at no pass over the f64 r.
 *   set-up     x_l for l >= 1 zero-filled once; q zero-filled once where the outer launch region is not the whole box.
 *              1. q = A(x), a plain launch in D   2. on Omega: r = b - q in D, outside +0; r32 = narrow(r), z32 = minv_0 * r32
 *              in S, +0 outside Omega for both through the same select; out of that launch rr_0 = sum r * r in D
 *              3. rr_0 is read back: rr_0 <= tol2 or max_iters == 0 returns with zero iterations (r, r32, z32 hold what step
 *              2 stored)   4. the rest of M32, which yields rz_0   5. p = widen(z32), whole box
 *   iteration  1. q = A(p) and pq = sum_Omega q * p out of the outer operator's dot-monitored launch
 *              2. alpha = rz / pq in D;  on all cells x = x + (alpha p), r = r - (alpha q), r32 = narrow(r) from the new r,
 *                 z32 = minv_0 * r32; out of that launch rr' = sum r * r in D
 *              3. the rest of M32, which yields rz'
 *              4. beta = rz' / rz;  on all cells p = widen(z32) + (beta p);  rz <- rz', rr <- rr'
 * As in neptune_hip_mgcg_solve: the breakdown rule (rz == 0 or pq == 0 gives alpha = beta = 0), the stop rule on the f64 rr,
 * check_every, trace (a DEVICE pointer to 3 * max_iters values of D), the fallback of step 1, the replay of one captured
 * iteration as a linear graph with its plain-launch fallback and NEPTUNE_HIP_MG_GRAPH=0, and cfg (the OUTER operator's launch
 * configuration).  neptune_hip_mgcg_rz0 and neptune_hip_mgcg_counts report on this entry as well.
 * LINE STAGES on levels >= 1 run through the unchanged cycle.  Stages on level 0: NEPTUNE_HIP_EUNSUPPORTED, nothing launched.
 * NEPTUNE_HIP_EINVAL, nothing launched: everything neptune_hip_mgcg_solve_lines refuses that applies; a dtype pair other than
 * (f64, f32); outer->g and levels[0].g disagreeing in rank, box or Omega; a null or misaligned work[i] or trace; any overlap
 * among outer's x, b, q, r, p, the trace and level 0's and level 1's x, b, q, minv; a factor field that overlaps a field the
 * solve writes in D; a stream that is being captured. */
int neptune_hip_mgcg_solve_mixed(const neptune_hip_mg_level_t *outer, int dtype_outer, neptune_hip_apply_dot_fn fn_dot,
                                 const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines, int n_levels,
                                 int dtype_inner, int sweeps, int coarse_sweeps, void *const work[2], int64_t max_iters,
                                 int64_t check_every, double tol2, void *trace, void *stream,
                                 const neptune_hip_launch_cfg_t *cfg, int64_t *iters_done, double *rr0, double *rr_last);
/* neptune_hip_mgcg_solve_mixed with the inner hierarchy's transfers chosen per pair, under the rule of
 * neptune_hip_mgcg_solve_transfer (symmetric pairs only; NULL or all-default is neptune_hip_mgcg_solve_mixed exactly, which is
 * this call with NULL); the same additional refusals. */
int neptune_hip_mgcg_solve_mixed_transfer(const neptune_hip_mg_level_t *outer, int dtype_outer, neptune_hip_apply_dot_fn fn_dot,
                                          const neptune_hip_mg_level_t *levels, const neptune_hip_mg_lines_t *lines,
                                          const neptune_hip_mg_transfer_t *transfer, int n_levels, int dtype_inner, int sweeps,
                                          int coarse_sweeps, void *const work[2], int64_t max_iters, int64_t check_every,
                                          double tol2, void *trace, void *stream, const neptune_hip_launch_cfg_t *cfg,
                                          int64_t *iters_done, double *rr0, double *rr_last);
/* neptune_hip_mg_smooth_dot with a wide sum, alone: the sweep in `dtype` exactly as neptune_hip_mg_smooth (the same bits in
 * x), and *dot_out = sum over Omega of widen(b) * widen(x_new) in `dtype_sum` -- each term exact.  (dtype, dtype_sum) =
 * (NEPTUNE_HIP_F32, NEPTUNE_HIP_F64) only.  dot_out: a DEVICE pointer to one double; otherwise as neptune_hip_mg_smooth_dot. */
int neptune_hip_mg_smooth_dot_wide(int dtype, int dtype_sum, const neptune_hip_apply_geom_t *g, const void *q, const void *b,
                                   const void *minv, void *x, void *dot_out, void *stream);
/* rz_0 = r . M(r) after the set-up of the last neptune_hip_mgcg_solve call of this process (0 when it was refused or ran
 * no iteration): with *rr0 and the trace, every scalar the recurrences used, so that a run can be replayed */
double neptune_hip_mgcg_rz0(void);
/* the last neptune_hip_mgcg_solve call of this process: iterations that ran as plain launches, iterations that ran as
 * graph launches, how many of all these took the fallback of step 1, and read-backs after blocks (the read of rr_0 is not
 * counted) */
void neptune_hip_mgcg_counts(int64_t *plain_iters, int64_t *graph_iters, int64_t *fallback_iters, int64_t *checks);

/* Which kernel neptune_hip_apply_builtin would run for (body, g, cfg):
 * NEPTUNE_HIP_KERNEL_DIRECT / _MARCH, or a negative error. */
int neptune_hip_apply_builtin_plan(int body, const neptune_hip_apply_geom_t *g,
                                   const void *const *in, const void *out,
                                   const neptune_hip_launch_cfg_t *cfg);

/* Name of the device kernel (as rocprofv3 lists it, without template arguments) that the
 * plan above launches; pointer valid for the process lifetime. */
const char *neptune_hip_kernel_name(int kernel);
/* Which march tile neptune_hip_apply_builtin would use for (body, g, cfg) if it plans the march kernel:
 * cfg->variant when valid, else the automatic choice (stencil shape, field size, launch region). */
int neptune_hip_apply_builtin_variant(int body, const neptune_hip_apply_geom_t *g,
                                      const neptune_hip_launch_cfg_t *cfg);
/* march tile variants compiled into the library, per field rank (2 or 3) */
int neptune_hip_march_variant_count(int rank);
const char *neptune_hip_march_variant_name(int rank, int variant);

/* ------------------------------------------------------------------------------------
 * 6. store (lib/Passes/DataflowLowering.cpp:165-220)
 *    no bounds : whole-buffer copy (memref.copy, :176-179)
 *    bounds    : logical box [lb,ub) copied between two buffers that each use their own
 *                logical origin (:184-217)
 * ---------------------------------------------------------------------------------- */
int neptune_hip_store_full(int dtype, const void *src, void *dst, int64_t count, void *stream);
int neptune_hip_store_box(int dtype, int rank, const void *src, const int64_t *src_lb,
                          const int64_t *src_ub, void *dst, const int64_t *dst_lb,
                          const int64_t *dst_ub, const int64_t *lb, const int64_t *ub,
                          void *stream);

/* ------------------------------------------------------------------------------------
 * 6b. reduce {kind = "sum"}  (lib/Passes/DataflowLowering.cpp:589-698; NeptuneIROps.td:272-299)
 *    Sum of the temp `src` (box [src_lb,src_ub)) over the logical domain [lb,ub) (NULL = the
 *    whole temp), accumulated in the element type and returned widened to double.  Blocking.
 *    The reference sums serially in row-major order; this is a fixed-tree parallel sum: bit-wise
 *    reproducible run to run, within 2(n-1) eps sum|x| of the serial result.
 * ---------------------------------------------------------------------------------- */
int neptune_hip_reduce_sum(int dtype, int rank, const void *src, const int64_t *src_lb,
                           const int64_t *src_ub, const int64_t *lb, const int64_t *ub,
                           double *result, void *stream);
/* reduce {kind = "sum" | "max" | "min" | "l1" | "l2"}: the same domain rules, error codes, blocking behaviour and
 * fixed tree as neptune_hip_reduce_sum, for every kind of the op (NeptuneIROps.td:266-288; the reference lowers only
 * "sum", so the other four are defined here).  Result in the element type T, widened to double (NaN,
 * +-inf and -0 survive the widening):
 *   SUM  sum x              empty domain: +0     the bits of neptune_hip_reduce_sum
 *   MAX  arith.maximumf     empty domain: -inf   NaN if any cell is NaN, -0 < +0; exact in any order
 *   MIN  arith.minimumf     empty domain: +inf   likewise
 *   L1   sum |x|            empty domain: +0     |x| exact, summed in T by the tree of SUM
 *   L2   sqrt(sum x*x)      empty domain: +0     x*x one rounding (no FMA), summed in T by the tree of SUM, one sqrt in T
 *                                                on the device, applied to the final sum
 * kind | NEPTUNE_HIP_REDUCE_RAW leaves the finishing step out (L2 returns sum x*x; the other kinds have none), for a
 * caller that combines the results of several boxes itself.  Any other kind: NEPTUNE_HIP_EINVAL, nothing launched. */
enum {
  NEPTUNE_HIP_REDUCE_SUM = 0,
  NEPTUNE_HIP_REDUCE_MAX = 1,
  NEPTUNE_HIP_REDUCE_MIN = 2,
  NEPTUNE_HIP_REDUCE_L1 = 3,
  NEPTUNE_HIP_REDUCE_L2 = 4,
  NEPTUNE_HIP_REDUCE_RAW = 0x100
};
int neptune_hip_reduce(int kind, int dtype, int rank, const void *src, const int64_t *src_lb,
                       const int64_t *src_ub, const int64_t *lb, const int64_t *ub,
                       double *result, void *stream);
/* device scratch of the reductions: (2048 + 1) elements of 8 bytes, owned by the library.  Used by the
 * fused apply+reduce kernels a lowered module carries (csrc/kernels/reduce_apply.hpp); calls that use it
 * are serialised by the stream they run on. */
void *neptune_hip_reduce_workspace(void);

/* ------------------------------------------------------------------------------------
 * 6c. vector updates for device-resident Krylov loops
 *    The reference's matrix-free solvers call the lowered operator from a host KSP loop over host Vecs
 *    (NeptunePETScRuntime.cpp:182-230, 719-786).  With device pointers in the memref arguments the operator and the
 *    dot products (reduce of an apply) already run without any host traffic; these two updates complete a solver
 *    loop that never leaves the GPU (a run-time scalar cannot enter a NeptuneIR apply region: IsolatedFromAbove).
 *    Element type of `a` follows dtype (rounded to float for F32).  Two roundings, no FMA.  Asynchronous.
 *      axpy: y[i] = y[i] + a * x[i]          xpay: y[i] = x[i] + a * y[i]
 * ---------------------------------------------------------------------------------- */
int neptune_hip_axpy(int dtype, int64_t n, double a, const void *x, void *y, void *stream);
int neptune_hip_xpay(int dtype, int64_t n, const void *x, double a, void *y, void *stream);

/* ------------------------------------------------------------------------------------
 * 7. helpers for tests and the bench (device-side, so 8 GiB fields never cross PCIe)
 * ---------------------------------------------------------------------------------- */
/* Deterministic field: value depends only on (global linear index + index_offset, seed);
 * integer hash mapped exactly to [-1,1) -- the same bits on host and device
 * (host twin: neptune_hip_hash_value). */
int neptune_hip_fill_hash(int dtype, void *dst, int64_t count, int64_t index_offset,
                          uint64_t seed, void *stream);
double neptune_hip_hash_value(int dtype, int64_t index, uint64_t seed);
/* Number of elements whose bit patterns differ between two device buffers (blocking). */
int64_t neptune_hip_count_mismatch(int dtype, const void *a, const void *b, int64_t count,
                                   void *stream);
/* Time `reps` launches of one built-in apply with HIP events on `stream`; returns the
 * average milliseconds per launch (blocking).  in/out as in neptune_hip_apply_builtin. */
double neptune_hip_time_apply_builtin(int body, const neptune_hip_apply_geom_t *g,
                                      const void *const *in, void *out, void *stream,
                                      const neptune_hip_launch_cfg_t *cfg, int warmup, int reps);
/* Plan-time tuning (in the spirit of FFTW_MEASURE): time every march tile of the library (and a
 * few chunk lengths) for exactly this geometry and these buffers, and return the fastest
 * configuration in *best (average ms per launch in *best_ms, may be NULL).  All candidates
 * produce identical bits; `out` ends up holding the result of a normal launch.  Blocking. */
int neptune_hip_autotune_builtin(int body, const neptune_hip_apply_geom_t *g, const void *const *in,
                                 void *out, void *stream, int reps, neptune_hip_launch_cfg_t *best,
                                 double *best_ms);
/* The same two calls for a lowered apply's geometry-level entry (`fn`, a module's <function>_<k>__geom): the
 * plan-time tuning a lowered module gets.  num_variants = how many march tiles that module holds
 * (its <function>_<k>__geom_variants(rank) export; the library's default tiles unless the module was built with
 * NEPTUNE_HIP_FULL_VARIANTS=1).  A tile that cannot take the geometry is rejected by the entry and skipped. */
double neptune_hip_time_apply_fn(neptune_hip_apply_fn fn, const neptune_hip_apply_geom_t *g,
                                 const void *const *in, void *out, void *stream,
                                 const neptune_hip_launch_cfg_t *cfg, int warmup, int reps);
int neptune_hip_autotune_fn(neptune_hip_apply_fn fn, int num_variants, const neptune_hip_apply_geom_t *g,
                            const void *const *in, void *out, void *stream, int reps,
                            neptune_hip_launch_cfg_t *best, double *best_ms);
/* ---- launch wisdom: measured launch choices, remembered across processes --------------------------------
 * An apply launched without an explicit configuration (cfg NULL or all-automatic) on a field of
 * NEPTUNE_HIP_TUNE_MIN_CELLS cells (default 2^24) or more measures ONCE which of its march tiles and chunk lengths is
 * fastest for exactly that (body, geometry): the first launch times the candidates (it synchronises the stream; every
 * candidate writes the same bits), later launches of the process reuse the choice, and the choice is appended to a
 * wisdom file so that every later PROCESS on the same device reuses it without timing anything (FFTW's wisdom, for
 * stencil launches).  File: $NEPTUNE_HIP_WISDOM, else <$NEPTUNE_CACHE_DIR or ~/.neptune/cache>/wisdom_v1.txt -- next
 * to the module cache; NEPTUNE_HIP_WISDOM= (empty) keeps choices in the process only.  NEPTUNE_HIP_TUNE=0 switches the
 * measuring off (fixed automatic tiles), NEPTUNE_HIP_TUNE=1 measures fields of any size.  A launch inside a stream
 * capture never measures.  Keys name the kernel build, the module and body, the element type and everything of the
 * geometry the launcher looks at; the library adds the device (name, architecture, CU count).
 * lookup: 1 = found (*cfg filled), 0 = unknown.  store: appends one line; 0 on success.
 * The reference has nothing to tune (one scalar loop nest, DataflowLowering.cpp:289-310). */
int neptune_hip_wisdom_lookup(const char *key, neptune_hip_launch_cfg_t *cfg);
int neptune_hip_wisdom_store(const char *key, const neptune_hip_launch_cfg_t *cfg, double ms);
/* the wisdom file of this process ("" when disabled); pointer valid for the process lifetime */
const char *neptune_hip_wisdom_path(void);
/* counters of this process: out[0] = first-use measurements made, out[1] = choices taken from the wisdom file,
 * out[2] = choices appended to it */
void neptune_hip_tune_stats(int64_t out[3]);
/* What the most recent apply launch of the calling thread really ran: kernel, march tile, planes per workgroup
 * (chunk as launched, never 0 for the march kernel).  Launchers call _note_launch; returns 0 if nothing was launched yet. */
void neptune_hip_note_launch(int kernel, int variant, int chunk);
int neptune_hip_last_launch(neptune_hip_launch_cfg_t *out);
/* Groups of sibling applies over shared inputs: counters of this process.  *fused = groups that ran as ONE
 * multi-output launch; *members_single = member applies of a group that ran as launches of their own (the plan has no
 * group form for the union footprint, a slab view is in force, or NEPTUNE_HIP_NO_GROUPS=1).  Lowered modules call
 * _note_group(fused, members) once per group they run. */
void neptune_hip_note_group(int fused, int members);
void neptune_hip_group_launch_counts(int64_t *fused, int64_t *members_single);

/* Plain 16-byte-per-lane device copy, timed the same way: the measured HBM ceiling.
 * mode selects the copy kernel shape (0 .. neptune_hip_copy_mode_count()-1: grid-stride, or
 * 1/2/4/8 loads in flight per lane with optional non-temporal loads/stores). */
double neptune_hip_time_copy(void *dst, const void *src, size_t bytes, void *stream, int mode,
                             int warmup, int reps);
int neptune_hip_copy_mode_count(void);

/* HIP events for callers that time a stream themselves (bench.py). */
void *neptune_hip_event_create(void);
void neptune_hip_event_destroy(void *ev);
void neptune_hip_event_record(void *ev, void *stream);
void neptune_hip_event_sync(void *ev);
double neptune_hip_event_elapsed_ms(void *start, void *stop);
/* make `stream` wait for `ev` (stream-to-stream ordering without blocking the host) */
void neptune_hip_stream_wait_event(void *stream, void *ev);

/* ------------------------------------------------------------------------------------
 * 8. slab decomposition across the GPUs of a node: halo exchange overlapped with the interior
 *    (the reference has no counterpart -- every PETSc object lives on PETSC_COMM_SELF,
 *    NeptunePETScRuntime.cpp:136,244,257).  One process per GPU.  Rank g owns planes [start_g, stop_g) of dim 0
 *    and keeps `radius` ghost planes per existing neighbour in the SAME dense buffer:
 *        local buffer = [ r_lo ghost planes | n_own owned planes | r_hi ghost planes ] x plane
 *    so a halo is one contiguous run of memory, sent and received in place.  No periodic wrap: at the global boundary
 *    r_lo / r_hi are 0 and the apply's copy-through semantics hold (DataflowLowering.cpp:283-287, 382-410).
 *    Two transports behind one communicator type:
 *      NEPTUNE_HIP_TRANSPORT_RCCL  ncclSend/ncclRecv, grouped, on a communication stream.  RCCL is loaded at the first
 *          call (dlopen librccl.so.1, reusing a copy already in the process); programs that never call these entry
 *          points never load it.
 *      NEPTUNE_HIP_TRANSPORT_PEER  the ranks of ONE node: every rank pushes its edge planes into its neighbour's ghost
 *          planes with hipMemcpyAsync through a mapping of the neighbour's buffer (hipIpcOpenMemHandle) -- SDMA engines
 *          over xGMI between two devices, no CU moves data -- and two one-wave kernels per exchange carry the
 *          "ghost planes free" / "planes landed" handshake through counters in a shared-memory segment
 *          (csrc/runtime/slab_peer.hpp).  Two processes may share one device on this transport.  Buffers exchanged
 *          through it must stay allocated while the communicator lives (their mappings are cached).
 *    Failures return NEPTUNE_HIP_ECOMM / NULL with the text in neptune_hip_slab_last_error() -- they never fall back to
 *    another transport.  Either transport issues work on a stream of its own: synchronise the compute stream (or wait
 *    for the plan's completion) before issuing collectives of ANOTHER communicator library on the same device
 *    (torch.distributed's, say) -- two communicators progressing concurrently can deadlock.
 *    Multi-rank runs of the RCCL transport between two devices are unverified on the authors' hardware (one-GPU boxes:
 *    loop-back and two-process tests only); a start-up exchange check like bench.py's is recommended.
 * ---------------------------------------------------------------------------------- */
#define NEPTUNE_HIP_SLAB_ID_BYTES 128
#define NEPTUNE_HIP_TRANSPORT_RCCL 0
#define NEPTUNE_HIP_TRANSPORT_PEER 1
typedef struct neptune_hip_slab_comm neptune_hip_slab_comm_t;
typedef struct neptune_hip_slab_plan neptune_hip_slab_plan_t;

/* rank 0 makes the id (RCCL: ncclGetUniqueId; peer: 128 random bytes naming the node's shared segment) and hands the
 * 128 bytes to every rank by any means.  The plain names are the RCCL transport. */
int neptune_hip_slab_unique_id(void *id_out);
int neptune_hip_slab_unique_id_ex(int transport, void *id_out);
/* collective over the `world` ranks (RCCL: ncclCommInitRank on the current device; peer: every rank maps the segment
 * and waits for the others, bounded by NEPTUNE_HIP_PEER_TIMEOUT_S, default 20 s); id may be NULL when world == 1 */
neptune_hip_slab_comm_t *neptune_hip_slab_comm_create(const void *id, int rank, int world);
neptune_hip_slab_comm_t *neptune_hip_slab_comm_create_ex(int transport, const void *id, int rank, int world);
void neptune_hip_slab_comm_destroy(neptune_hip_slab_comm_t *comm);
const char *neptune_hip_slab_last_error(void);
/* "rccl" / "peer" */
const char *neptune_hip_slab_comm_transport(const neptune_hip_slab_comm_t *comm);
/* NEPTUNE_HIP_OK, or NEPTUNE_HIP_ECOMM once a device-side wait of the peer transport has timed out (a neighbour died
 * or fell more than the timeout behind): every exchange since then left stale ghost planes.  Never blocks. */
int neptune_hip_slab_comm_status(neptune_hip_slab_comm_t *comm);

/* Refresh the ghost planes of one local buffer on `stream`: the first r_lo owned planes go to peer_lo and its last
 * planes arrive in my lower ghosts; likewise r_hi / peer_hi above (a side with 0 ghost planes is skipped, its peer is
 * ignored).  Asynchronous.  peer == own rank is allowed (a loop-back used by the single-GPU tests: RCCL matches the
 * two send/receive pairs in order, so the lower ghosts receive the rank's FIRST owned planes; the peer transport
 * pushes to the neighbour's opposite side, so they receive its LAST owned planes -- a periodic wrap).
 * _many: the ghost planes of `nfields` buffers (<= NEPTUNE_HIP_MAX_INPUTS) in one grouped exchange / one handshake. */
int neptune_hip_halo_exchange(neptune_hip_slab_comm_t *comm, void *field, size_t plane_bytes, int64_t n_own,
                              int r_lo, int r_hi, int peer_lo, int peer_hi, void *stream);
int neptune_hip_halo_exchange_many(neptune_hip_slab_comm_t *comm, void *const *fields, const size_t *plane_bytes,
                                   int nfields, int64_t n_own, int r_lo, int r_hi, int peer_lo, int peer_hi,
                                   void *stream);

/* One apply over this rank's slab, planned once.  `fn`: a lowered apply's geometry-level entry, or NULL to use
 * built-in body `body`.  `local`: the geometry of the LOCAL buffers (boxes include the ghost planes; apply.bounds
 * already clipped to the owned planes; the region is ignored).  radius = the apply's reach along dim 0.
 * neptune_hip_slab_apply then runs, per call:
 *     comm stream   : wait for the input on `compute_stream`, exchange the ghost planes of EVERY input
 *                     (a stream of the greatest priority the device offers: the exchange is dispatched ahead of the
 *                     interior grid, which fills every CU)
 *     compute stream: interior planes (those that need no ghost data)                 -- overlaps the exchange
 *     compute stream: wait for the exchange, then the `radius` edge planes per side that has a neighbour
 * overlap = 0 makes the interior wait for the exchange as well (debugging).  Asynchronous on compute_stream. */
neptune_hip_slab_plan_t *neptune_hip_slab_plan_create(neptune_hip_slab_comm_t *comm, neptune_hip_apply_fn fn, int body,
                                                      int dtype, const neptune_hip_apply_geom_t *local, int radius,
                                                      int r_lo, int r_hi, int peer_lo, int peer_hi,
                                                      const neptune_hip_launch_cfg_t *cfg);
int neptune_hip_slab_apply(neptune_hip_slab_plan_t *plan, const void *const *in, void *out, void *compute_stream,
                           int overlap);
void neptune_hip_slab_plan_destroy(neptune_hip_slab_plan_t *plan);
/* Where a sharded step spends its time.  _timing(plan, 1) makes every following neptune_hip_slab_apply record five
 * timed events (a ring of 64 steps; no synchronisation is added); _timing_read waits for the recorded steps and
 * returns their averages in milliseconds:
 *   out[0] exchange   (communication stream: input ready -> ghost planes landed)
 *   out[1] interior   (compute stream: the interior launch)
 *   out[2] edge wait  (how long after the interior's end the exchange ended; 0 when it was hidden behind it)
 *   out[3] edges      (the edge launches)
 *   out[4] step       (interior start -> edges done)
 *   out[5] steps averaged */
int neptune_hip_slab_plan_timing(neptune_hip_slab_plan_t *plan, int on);
int neptune_hip_slab_plan_timing_read(neptune_hip_slab_plan_t *plan, double out[6]);

#ifdef __cplusplus
}
#endif
#endif /* NEPTUNE_HIP_H */
