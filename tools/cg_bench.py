#!/usr/bin/env python3
"""What a conjugate-gradient iteration costs: ONE measurement per process, warmed up, device-resident f64
vectors, the 7-point Poisson operator of examples/cg_matrix_free.py.

  --mode loop      the caller-side loop of examples/cg_matrix_free.py: lowered matmult, fused reduce(apply(a*b)) dot products,
                   torch updates, two blocking read-backs per iteration.  Uses nothing this feature added, so it runs
                   unchanged against a build of the parent commit: --root <that tree>.
  --mode solver    neptune_hip.apply.cg_solve with --check-every (this build only); --dot fallback: its fallback path
  --mode geom      the operator's plain <fn>__geom launch alone (both builds): what the feature must not slow down
  --mode dot       the dot-monitored launch alone against ...
  --mode dot2      ... a plain launch plus neptune_hip_dot (this build only): which one an operator class should take

  --n N --iters K --root DIR

Timing: loop / solver: wall clock around exactly K iterations (the tolerance is unreachable), after one warm-up solve of the
same length, synchronised before and after; geom / dot / dot2: HIP events around K launches after 5.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["loop", "solver", "geom", "dot", "dot2"], required=True)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--dot", choices=["auto", "fallback"], default="auto")
    ap.add_argument("--root", default=str(HERE.parent))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(root / "examples")]
    os.environ["NEPTUNE_HIP_LIB"] = str(root / "neptune-pde-solver_amd" / "lib" / "libneptune_hip.so")
    import torch
    import cg_matrix_free as ex
    from neptune_hip import _capi, apply, fields, lowering
    _capi.load().neptune_hip_init(0)
    n, K = args.n, args.iters
    shape = (n, n, n)
    interior = ([1, 1, 1], [n - 1] * 3)
    new_api = args.mode in ("solver", "dot", "dot2")
    mod = lowering.compile_module(ex.module_text(shape), **({"dot_entries": True} if new_api else {}))
    gen = torch.Generator(device="cuda").manual_seed(7)
    b = torch.zeros(shape, dtype=torch.float64, device="cuda")
    b[1:-1, 1:-1, 1:-1] = torch.rand((n - 2,) * 3, dtype=torch.float64, device="cuda", generator=gen)
    field = lambda t: fields.DeviceField((0, 0, 0), shape, _capi.F64, t)
    out = {"label": args.label, "mode": args.mode, "n": n, "iters": K}

    if args.mode == "loop":
        run = lambda: ex.cg(lambda y, v: mod.call("matmult", y, v), lambda u, v: mod.call("dot", u, v), b, torch.zeros_like(b),
                            tol=0.0, maxit=K)
    elif args.mode == "solver":
        entry = mod.dot_entry(next(a["function"] for a in mod.report["applies"] if a.get("dot_symbol")))
        work = [field(torch.empty_like(b)) for _ in range(3)]
        run = lambda: apply.cg_solve(entry, field(torch.zeros_like(b)), field(b), interior, K, -1.0, check_every=args.check_every,
                                     dot=args.dot, work=work)
        out.update(check_every=args.check_every, dot=args.dot)
    if args.mode in ("loop", "solver"):
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        out["ms_per_iteration"] = round((time.perf_counter() - t0) * 1e3 / K, 5)
        out["iterations_run"] = int(res[1] if args.mode == "loop" else res[0])
        if args.mode == "solver":
            out["counts"] = list(apply.cg_counts())
    else:
        fn = next(a["function"] for a in mod.report["applies"] if a.get("geom_symbol"))
        entry = mod.dot_entry(fn) if new_api else mod.geom_entry(fn)
        p, q = field(b), field(torch.empty_like(b))
        scalar = torch.zeros(1, dtype=torch.float64, device="cuda")

        def step():
            if args.mode == "dot":
                apply.apply_dot(entry, [p], q, interior, dot_out=scalar)
            else:
                apply.apply_builtin(entry, [p], q, interior)
                if args.mode == "dot2":
                    apply.dot(q, p, interior, dot_out=scalar)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(K):
            step()
        e1.record()
        torch.cuda.synchronize()
        out["ms_per_launch"] = round(e0.elapsed_time(e1) / K, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
