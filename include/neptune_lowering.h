/*
 * neptune_lowering.h -- C ABI of libneptune_lowering.so: the NeptuneIR -> HIP lowering as a
 * library (the `neptune-opt --neptuneir-to-hip` tool is a thin main() over the same calls).
 *
 * Takes the place, for the stencil hot path, of the reference's pass pipeline entry points
 * buildNeptuneToLLVMPipeline / NeptuneCompiler::runPipeline + compileToObjectFile
 * (lib/Pipeline/NeptuneIRPassesPipeline.cpp:5-47, lib/Compiler/NeptuneCompiler.cpp:291-358).
 * All strings returned through char** are malloc'ed; release them with neptune_lowering_free.
 * Return value: 0 on success, negative on failure (then *diag_out holds "line N: message").
 */
#ifndef NEPTUNE_LOWERING_H
#define NEPTUNE_LOWERING_H
#ifdef __cplusplus
extern "C" {
#endif

/* Parse + verify only (ApplyOp::verify, checkApplyLike, linear_opdef body rules;
 * reference lib/Dialect/NeptuneIR/NeptuneIRVerifier.cpp:34-171, lib/Passes/VerifyAndAnnotate.cpp:87-214). */
int neptune_lowering_verify(const char *mlir_text, char **diag_out);

/* Lower a module to one HIP translation unit.  *report_out is a JSON object:
 *   lowered     exported symbols
 *   signatures  per symbol: argument/result kinds, element types, ranks, shapes, origins
 *   skipped     functions left alone (solver ops and implicit time stepping: they stay on the host path)
 *   applies     per neptune_ir.apply (and per explicit time_advance): rank, inputs, element type, kernel family
 *               (march | direct | reduce = evaluated inside the consuming reduce's kernel), stencil shape,
 *               halo0 (reach along dim 0: the ghost planes a slab decomposition must hold) and geom_symbol,
 *               the exported geometry-level entry of that apply (neptune_hip_apply_fn, include/neptune_hip.h);
 *               leapfrog_symbol, the pair entry <geom_symbol>L2 of a two-level scheme (neptune_hip_leapfrog2_fn), or ""
 *               norm_symbol (only with the option below), the monitored launch <geom_symbol>N (neptune_hip_apply_norm_fn)
 *               dot_symbol (only with its option below), the dot-monitored launch <geom_symbol>D (neptune_hip_apply_dot_fn)
 * Lowering options travel in the module text, one comment line each: "// neptune-hip-option: <name>".
 *   norm-entries   every apply whose input 0 has the result's element type and a box equal to the result's (a fused
 *                  explicit Euler step included) also exports its monitored launch <function>_<k>__geomN: the apply and
 *                  the update norm sum (new - old)^2 from one launch (include/neptune_hip.h).  Without it
 *                  source and report are what they are without this feature.  neptune-opt: --norm-entries; Python:
 *                  compile_module(..., norm_entries=True).
 *   dot-entries    the applies norm-entries names also export their dot-monitored launch <function>_<k>__geomD: the apply and
 *                  sum new * in[0] from one launch -- p . A(p) for a conjugate-gradient iteration (include/neptune_hip.h,
 *                  DESIGN.md 3.11).  Without it source and report are what they are without this feature.  neptune-opt:
 *                  --dot-entries; Python: compile_module(..., dot_entries=True).
 *   reduce-kinds   neptune_ir.reduce kinds "max" | "min" | "l1" | "l2" verify and lower (semantics: DESIGN.md 3.3; any other
 *                  kind: 'neptune_ir.reduce' op unsupported reduce kind "<k>"); every reduce then goes through the kind-taking
 *                  runtime forms, and the report entry of an apply fused into a reduce carries "reduce_kind".  Without it a
 *                  kind other than "sum" fails verification with the reference's diagnostic, and source and report are what
 *                  they are without this feature.  neptune-opt: --reduce-kinds; Python: to_hip / verify /
 *                  compile_module(..., reduce_kinds=True); modules built with neptune.reduce_max / _min / _l1 / _l2 carry
 *                  the line themselves.
 * Set NEPTUNE_HIP_FULL_VARIANTS=1 in the environment of neptune_lowering_compile to build every march tile
 * into the module instead of the defaults (for NEPTUNE_HIP_TUNE=1). */
int neptune_lowering_to_hip(const char *mlir_text, char **source_out, char **report_out, char **diag_out);

/* Lower and compile to a shared object with hipcc (--offload-arch=gfx950 -ffp-contract=off),
 * linked against <repo_root>/neptune-pde-solver_amd/lib/libneptune_hip.so.  The emitted source is
 * kept next to the library as <so_path>.hip.  hipcc may be NULL (/opt/rocm/bin/hipcc). */
int neptune_lowering_compile(const char *mlir_text, const char *so_path, const char *repo_root,
                             const char *hipcc, char **report_out, char **diag_out);

void neptune_lowering_free(char *p);
const char *neptune_lowering_version(void);

#ifdef __cplusplus
}
#endif
#endif
