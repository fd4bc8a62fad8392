#!/usr/bin/env python3
"""What the Jacobi preconditioner costs per iteration: cg_solve and cg_solve(minv=...) alternated in one job on
the reaction-diffusion operator of examples/pcg_variable_coeff.py, f64, a fixed number of iterations (tol2 = 0 is never
reached), and -- with --parent-root -- cg_solve of a build of the parent commit alternated with both.

  tools/pcg_bench.py [--sizes 256,512] [--reps 4] [--iters 50] [--check-every 10] [--parent-root DIR] [--limit SECONDS]

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.  Order per
size: repetition by repetition, parent's cg_solve (if asked for), cg_solve, preconditioned -- so drift hits all alike.

  --one --mode cg|pcg --n N [--root DIR]      one measurement (what a child runs): one warm-up solve of the same length, then
                                              wall clock around exactly --iters iterations, synchronised before and after;
                                              prints one JSON line

Yardsticks printed at the end, per size: the preconditioned solve's time per iteration against cg_solve's times 13 / 11 (the
ratio of field passes), margin: the spread (max - min) of cg_solve's repetitions; cg_solve against the parent's, margin: the
parent's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent


def one(args):
    root = Path(args.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(HERE.parent / "examples")]
    os.environ["NEPTUNE_HIP_LIB"] = str(root / "neptune-pde-solver_amd" / "lib" / "libneptune_hip.so")
    import torch
    # the packages of --root first: the example module puts its own tree in front of sys.path when it is imported, and what
    # is imported by then stays
    import neptune  # noqa: F401  (the DSL build_text uses)
    import neptune_hip
    from neptune_hip import _capi, apply, fields, lowering
    import pcg_variable_coeff as ex
    for mod in (neptune, neptune_hip, _capi, apply, fields, lowering):
        if root not in Path(mod.__file__).resolve().parents:
            raise SystemExit(f"{mod.__name__} was imported from {mod.__file__}, not from --root {root}")
    _capi.load().neptune_hip_init(0)
    n, K = args.n, args.iters
    text, interior = ex.build_text(n)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    shape = (n, n, n)
    gen = torch.Generator(device="cuda").manual_seed(7)
    pick = torch.randint(0, 4, shape, device="cuda", generator=gen)
    w = torch.tensor(ex.W_VALUES, dtype=torch.float64, device="cuda")[pick]
    b = torch.zeros(shape, dtype=torch.float64, device="cuda")
    b[1:-1, 1:-1, 1:-1] = torch.rand((n - 2,) * 3, dtype=torch.float64, device="cuda", generator=gen)
    del pick
    field = lambda t: fields.DeviceField((0, 0, 0), shape, _capi.F64, t)
    wf, bf, x = field(w), field(b), field(torch.zeros_like(b))
    work = [field(torch.empty_like(b)) for _ in range(3)]
    kw = {}
    if args.mode == "pcg":
        kw["minv"] = apply.jacobi_minv(entry, x, interior, others=[wf])

    def run():
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = apply.cg_solve(entry, x, bf, interior, K, 0.0, check_every=args.check_every, others=[wf], work=work, **kw)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0
    run()
    res, seconds = run()
    print(json.dumps({"label": args.label, "mode": args.mode, "n": n, "iters": K, "check_every": args.check_every,
                      "iterations_run": int(res[0]), "rr0": res[1], "rr_last": res[2], "counts": list(apply.cg_counts()),
                      "ms_per_iteration": round(seconds * 1e3 / K, 5), "package": str(Path(neptune_hip.__file__).resolve().parent),
                      "library": str(_capi.library_path())}))


def drive(args):
    sizes = [int(s) for s in args.sizes.split(",")]
    kinds = ([("parent cg", "cg", args.parent_root)] if args.parent_root else []) + [("cg", "cg", str(HERE.parent)), ("pcg", "pcg", str(HERE.parent))]
    results = {}
    for n in sizes:
        for rep in range(args.reps):
            for label, mode, root in kinds:
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--one", "--mode", mode,
                       "--n", str(n), "--iters", str(args.iters), "--check-every", str(args.check_every), "--root", root,
                       "--label", label]
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    print(f"{label} n={n} repetition {rep}: exit status {p.returncode}; nothing more is started", flush=True)
                    return p.returncode
                out = json.loads(p.stdout.strip().splitlines()[-1])
                if out["iterations_run"] != args.iters:
                    print(f"{label} n={n}: ran {out['iterations_run']} iterations, not {args.iters}", flush=True)
                    return 1
                print(json.dumps(out), flush=True)
                results.setdefault((n, label), []).append(out["ms_per_iteration"])
    for n in sizes:
        stat = {}
        for label, _, _ in kinds:
            v = results[(n, label)]
            stat[label] = (statistics.median(v), max(v) - min(v))
            print(f"{n}^3 f64 {label:>9}: {stat[label][0]:.4f} ms per iteration (median of {len(v)}), spread {stat[label][1]:.4f} "
                  f"({min(v):.4f} .. {max(v):.4f})")
        cg, spread = stat["cg"]
        yard = cg * 13.0 / 11.0
        print(f"{n}^3 f64: pcg {stat['pcg'][0]:.4f} against cg x 13/11 = {yard:.4f}, margin {spread:.4f}: "
              f"{'within' if stat['pcg'][0] <= yard + spread else 'ABOVE'} (pcg / cg = {stat['pcg'][0] / cg:.3f})")
        if "parent cg" in stat:
            par, pspread = stat["parent cg"]
            print(f"{n}^3 f64: cg {cg:.4f} against the parent's {par:.4f}, margin {pspread:.4f}: "
                  f"{'within' if cg <= par + pspread else 'ABOVE'}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--mode", choices=["cg", "pcg"], default="pcg")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--root", default=str(HERE.parent))
    ap.add_argument("--label", default="")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--limit", type=int, default=180)
    args = ap.parse_args()
    if args.one:
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
