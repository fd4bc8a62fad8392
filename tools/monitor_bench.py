#!/usr/bin/env python3
"""What a checked step costs: ONE measurement per process, warmed up, device-resident f64 fields.

  --mode monitored   the apply and S = sum (new - old)^2 from one launch: <fn>__geomN (this build only)
  --mode plain       the apply alone: <fn>__geom
  --mode twopass     the best a build WITHOUT monitored launches can do for the same quantity: one __geom launch, then the
                     fused reduce(apply((a - b) * (a - b))) of a lowered two-input module over both fields -- four field
                     passes per checked step instead of two.  Uses nothing this feature added, so it runs unchanged against
                     a build of the parent commit: --root <that tree>.
  --mode fallback    this build's own fallback: __geom, then neptune_hip_update_norm

  --kind 3d7|2d5  --n N        7-point N^3 or 5-point N^2 (the committed fixtures' operators)
  --root DIR                   the tree whose package and libraries are measured (default: this one)

Timing: HIP events around `--reps` back-to-back steps after `--warmup` steps, on the current stream; the scalar stays on the
device (monitored / fallback) or comes back per step as the lowered function's result (twopass: its reduce synchronises,
as it would in a real loop).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent

DIFFSQ = '''
#l = #neptune_ir.location<"cell">
!t = !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [{zeros}], ub = [{shape}]>, location = #l>
!f = !neptune_ir.field<element = f64, bounds = #neptune_ir.bounds<lb = [{zeros}], ub = [{shape}]>, location = #l>
module {{
  func.func @diffsq(%a: memref<{mr}>, %b: memref<{mr}>) -> f64 {{
    %fa = neptune_ir.wrap %a : memref<{mr}> -> !f
    %fb = neptune_ir.wrap %b : memref<{mr}> -> !f
    %u = neptune_ir.load %fa : !f -> !t
    %v = neptune_ir.load %fb : !f -> !t
    %sq = neptune_ir.apply(%u, %v) attributes {{bounds = #neptune_ir.bounds<lb = [{ones}], ub = [{inner}]>}} : (!t, !t) -> !t {{
      ^bb0({idx}, %x: !t, %y: !t):
        %p = neptune_ir.access %x[{zeros}] : !t -> f64
        %q = neptune_ir.access %y[{zeros}] : !t -> f64
        %d = arith.subf %p, %q : f64
        %e = arith.mulf %d, %d : f64
        neptune_ir.yield %e : f64
    }}
    %s = neptune_ir.reduce %sq in #neptune_ir.bounds<lb = [{ones}], ub = [{inner}]> {{kind = "sum"}} : !t -> f64
    func.return %s : f64
  }}
}}
'''


def diffsq_module(shape):
    rank = len(shape)
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    return DIFFSQ.format(zeros=lst([0] * rank), shape=lst(shape), ones=lst([1] * rank), inner=lst([n - 1 for n in shape]),
                         mr="x".join(["?"] * rank) + "xf64", idx=", ".join(f"%i{d}: index" for d in range(rank)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["monitored", "plain", "twopass", "fallback"], required=True)
    ap.add_argument("--kind", choices=["3d7", "2d5"], default="3d7")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--root", default=str(HERE.parent))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(root / "tools")]
    os.environ["NEPTUNE_HIP_LIB"] = str(root / "neptune-pde-solver_amd" / "lib" / "libneptune_hip.so")
    import ctypes as C
    import torch
    from make_stencil_mlir import stencil_module
    from neptune_hip import _capi, apply, fields, lowering
    lib = _capi.load()
    lib.neptune_hip_init(0)
    shape = (args.n,) * (3 if args.kind == "3d7" else 2)
    bounds = ([1] * len(shape), [n - 1 for n in shape])
    text = stencil_module(args.kind, shape)
    opname = {"3d7": "lap3d", "2d5": "lap2d"}[args.kind]
    t0 = time.time()
    if args.mode == "monitored":
        mod = lowering.compile_module(text, norm_entries=True)
        entry = mod.norm_entry(opname)
    else:
        mod = lowering.compile_module(text)
        entry = mod.geom_entry(opname)
    red = lowering.compile_module(diffsq_module(shape)) if args.mode == "twopass" else None
    compile_s = time.time() - t0
    a = fields.DeviceField.hashed(shape, _capi.F64, seed=1)
    b = fields.DeviceField.empty_like(a)
    b.tensor.copy_(a.tensor)
    scalar = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = apply.geom_for([a], b, bounds)
    st = fields.current_stream_ptr()
    last = [0.0]

    def step():
        if args.mode == "monitored":
            apply.apply_norm(entry, [a], b, bounds, sum_out=scalar)
        else:
            apply.apply_builtin(entry, [a], b, bounds)
            if args.mode == "twopass":
                last[0] = red.call("diffsq", b.tensor, a.tensor)
            elif args.mode == "fallback":
                _capi.check(lib.neptune_hip_update_norm(_capi.F64, C.byref(g), b.ptr, a.ptr, scalar.data_ptr(), st), "update_norm")

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    value = last[0] if args.mode == "twopass" else (float(scalar.item()) if args.mode != "plain" else None)
    cfg = _capi.LaunchCfg()
    lib.neptune_hip_last_launch(C.byref(cfg))
    print(json.dumps({"label": args.label, "mode": args.mode, "kind": args.kind, "n": args.n, "ms_per_step": round(ms, 5),
                      "S": value, "reps": args.reps, "compile_s": round(compile_s, 1),
                      "last_launch": [cfg.kernel, cfg.variant, cfg.chunk]}))


if __name__ == "__main__":
    main()
