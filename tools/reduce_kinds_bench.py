#!/usr/bin/env python3
"""What a reduce of each kind costs: ONE measurement per process, warmed up, device-resident fields.

  --form plain    neptune_hip.apply.reduce(field, kind) -- for --kind sum neptune_hip.apply.reduce_sum, which every build has
  --form fused    a lowered reduce(apply) over two fields: --kind sum is reduce_sum(apply(a * b)), the dot product (no lowering
                  option: a build of the parent commit lowers it too); the other kinds reduce apply(|a - b|)
  --kind sum|max|min|l1|l2     --dtype f64|f32     --n N (an N^3 field)     --box whole|interior
  --root DIR      the tree whose package and libraries are measured (default: this one).  The yardstick of both claims is
                  `--kind sum` with --root pointing at a built checkout of the parent commit.

Timing: HIP events around `--reps` back-to-back reduces after `--warmup`, on the current stream.  Every reduce is blocking
(its scalar comes back to the host), as it is in a real loop, so a figure holds the launch pair, the 8-byte copy and the
synchronisation.  Prints one JSON line: ms per reduce and the bytes read per second.  profiles/reduce_kinds.txt holds the
method that alternates the yardstick with the kinds."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent

FUSED = '''{option}#l = #neptune_ir.location<"cell">
!t = !neptune_ir.temp<element = {e}, bounds = #neptune_ir.bounds<lb = [0, 0, 0], ub = [{n}, {n}, {n}]>, location = #l>
!f = !neptune_ir.field<element = {e}, bounds = #neptune_ir.bounds<lb = [0, 0, 0], ub = [{n}, {n}, {n}]>, location = #l>
module {{
  func.func @red(%a: memref<?x?x?x{e}>, %b: memref<?x?x?x{e}>) -> {e} {{
    %fa = neptune_ir.wrap %a : memref<?x?x?x{e}> -> !f
    %fb = neptune_ir.wrap %b : memref<?x?x?x{e}> -> !f
    %u = neptune_ir.load %fa : !f -> !t
    %v = neptune_ir.load %fb : !f -> !t
    %w = neptune_ir.apply(%u, %v) attributes {{bounds = #neptune_ir.bounds<lb = [0, 0, 0], ub = [{n}, {n}, {n}]>}} : (!t, !t) -> !t {{
      ^bb0(%i: index, %j: index, %k: index, %x: !t, %y: !t):
        %p = neptune_ir.access %x[0, 0, 0] : !t -> {e}
        %q = neptune_ir.access %y[0, 0, 0] : !t -> {e}
{body}
        neptune_ir.yield %r : {e}
    }}
    %s = neptune_ir.reduce %w in #neptune_ir.bounds<lb = [{lo}, {lo}, {lo}], ub = [{hi}, {hi}, {hi}]> {{kind = "{kind}"}} : !t -> {e}
    func.return %s : {e}
  }}
}}
'''


def fused_module(kind, elem, n, lo, hi):
    if kind == "sum":
        body, option = f"        %r = arith.mulf %p, %q : {elem}", ""
    else:
        body = f"        %d = arith.subf %p, %q : {elem}\n        %r = math.absf %d : {elem}"
        option = "// neptune-hip-option: reduce-kinds\n"
    return FUSED.format(option=option, e=elem, n=n, lo=lo, hi=hi, kind=kind, body=body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["plain", "fused"], default="plain")
    ap.add_argument("--kind", choices=["sum", "max", "min", "l1", "l2"], required=True)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--box", choices=["whole", "interior"], default="whole")
    ap.add_argument("--root", default=str(HERE.parent))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(root / "tools")]
    os.environ["NEPTUNE_HIP_LIB"] = str(root / "neptune-pde-solver_amd" / "lib" / "libneptune_hip.so")
    import torch
    from neptune_hip import _capi, apply, fields, lowering
    _capi.load().neptune_hip_init(0)
    n = args.n
    dt = _capi.F64 if args.dtype == "f64" else _capi.F32
    esize = 8 if args.dtype == "f64" else 4
    lo, hi = (0, n) if args.box == "whole" else (1, n - 1)
    a = fields.DeviceField.hashed((n, n, n), dt, seed=1)
    t0 = time.time()
    if args.form == "plain":
        bounds = None if args.box == "whole" else ([lo] * 3, [hi] * 3)
        if args.kind == "sum":
            run = lambda: apply.reduce_sum(a, bounds)
        else:
            run = lambda: apply.reduce(a, args.kind, bounds)
        fields_read = 1
    else:
        b = fields.DeviceField.hashed((n, n, n), dt, seed=2)
        mod = lowering.compile_module(fused_module(args.kind, args.dtype, n, lo, hi))
        run = lambda: mod.call("red", a.tensor, b.tensor)
        fields_read = 2
    compile_s = time.time() - t0
    value = None
    for _ in range(args.warmup):
        value = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        value = run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    nbytes = fields_read * (hi - lo) ** 3 * esize
    print(json.dumps({"label": args.label, "form": args.form, "kind": args.kind, "dtype": args.dtype, "n": n, "box": args.box,
                      "ms": round(ms, 5), "TBps": round(nbytes / ms / 1e9, 3), "value": value, "reps": args.reps,
                      "compile_s": round(compile_s, 1)}))


if __name__ == "__main__":
    main()
