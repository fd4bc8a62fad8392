#!/usr/bin/env python3
"""What device-resident BiCGStab costs per iteration: apply.bicgstab_solve, a caller-side BiCGStab built from what
the library had before it (plain launch, apply.apply_dot, torch updates, four blocking read-backs per iteration) and cg_solve
alternated in one job on the upwind advection-diffusion operator of examples/advection_diffusion_implicit.py, f64, a fixed
number of iterations (tol2 = 0 is never reached), and -- with --parent-root -- cg_solve of a build of the parent commit
alternated with them.  (cg_solve does not converge on this operator; a fixed number of its iterations costs what it costs.)

  tools/bicgstab_bench.py [--sizes 256,512] [--reps 4] [--iters 50] [--check-every 10] [--parent-root DIR] [--limit SECONDS]

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.  Order per
size: repetition by repetition, parent's cg_solve (if asked for), cg_solve, the caller-side loop, bicgstab_solve -- so drift
hits all alike.

  --one --mode cg|caller|bicgstab --n N [--root DIR]   one measurement (what a child runs): one warm-up solve of the same length,
                                              then wall clock around exactly --iters iterations, synchronised before and after;
                                              prints one JSON line

Yardsticks printed at the end, per size: (a) bicgstab_solve's time per iteration against the caller-side loop's, margin: the
spread (max - min) of that loop's repetitions; (b) cg_solve against the parent's, margin: the parent's spread; (c)
bicgstab_solve against cg_solve's times 21 / 11 (the ratio of field passes): reported."""
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
    import advection_diffusion_implicit as ex
    for mod in (neptune, neptune_hip, _capi, apply, fields, lowering):
        if root not in Path(mod.__file__).resolve().parents:
            raise SystemExit(f"{mod.__name__} was imported from {mod.__file__}, not from --root {root}")
    _capi.load().neptune_hip_init(0)
    n, K = args.n, args.iters
    text, interior = ex.build_text(n)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    shape = (n, n, n)
    gen = torch.Generator(device="cuda").manual_seed(7)
    b = torch.zeros(shape, dtype=torch.float64, device="cuda")
    b[1:-1, 1:-1, 1:-1] = torch.rand((n - 2,) * 3, dtype=torch.float64, device="cuda", generator=gen)
    field = lambda t: fields.DeviceField((0, 0, 0), shape, _capi.F64, t)
    bf, x = field(b), field(torch.zeros_like(b))
    work = [field(torch.empty_like(b)) for _ in range(5)]

    def caller_side():
        """BiCGStab from the pieces the library had before the solver: every scalar crosses to the host"""
        r, rh, p, v, t = (w.tensor for w in work)
        apply.apply_builtin(entry, [x], work[3], interior)
        r.zero_()
        r[1:-1, 1:-1, 1:-1] = b[1:-1, 1:-1, 1:-1] - v[1:-1, 1:-1, 1:-1]
        rh.copy_(r)
        p.copy_(r)
        rho = rr0 = float(torch.sum(r * r))
        rr = rr0
        for _ in range(K):
            apply.apply_builtin(entry, [work[2]], work[3], interior)
            rv = float(torch.sum(rh * v))
            alpha = 0.0 if (rho == 0.0 or rv == 0.0) else rho / rv
            r.sub_(v, alpha=alpha)
            ts = apply.apply_dot(entry, [work[0]], work[4], interior)
            tt = float(torch.sum(t * t))
            omega = 0.0 if tt == 0.0 else ts / tt
            x.tensor.add_(p, alpha=alpha).add_(r, alpha=omega)
            r.sub_(t, alpha=omega)
            rho_new, rr = float(torch.sum(rh * r)), float(torch.sum(r * r))
            beta = 0.0 if (rho == 0.0 or rv == 0.0 or omega == 0.0) else (rho_new / rho) * (alpha / omega)
            p.sub_(v, alpha=omega).mul_(beta).add_(r)
            rho = rho_new
        return (K, rr0, rr)

    def run():
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.mode == "cg":
            res = apply.cg_solve(entry, x, bf, interior, K, 0.0, check_every=args.check_every, work=work[:3])
        elif args.mode == "caller":
            res = caller_side()
        else:
            res = apply.bicgstab_solve(entry, x, bf, interior, K, 0.0, check_every=args.check_every, work=work)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0
    run()
    res, seconds = run()
    print(json.dumps({"label": args.label, "mode": args.mode, "n": n, "iters": K, "check_every": args.check_every,
                      "iterations_run": int(res[0]), "rr0": res[1], "rr_last": res[2], "counts": list(apply.cg_counts()) if args.mode != "caller" else None,
                      "ms_per_iteration": round(seconds * 1e3 / K, 5), "package": str(Path(neptune_hip.__file__).resolve().parent),
                      "library": str(_capi.library_path())}))


def drive(args):
    sizes = [int(s) for s in args.sizes.split(",")]
    here = str(HERE.parent)
    kinds = ([("parent cg", "cg", args.parent_root)] if args.parent_root else []) + [("cg", "cg", here), ("caller", "caller", here),
                                                                                     ("bicgstab", "bicgstab", here)]
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
        cg, _ = stat["cg"]
        bi = stat["bicgstab"][0]
        caller, cspread = stat["caller"]
        print(f"{n}^3 f64: (a) bicgstab {bi:.4f} against the caller-side loop's {caller:.4f}, margin {cspread:.4f}: "
              f"{'below' if bi < caller - cspread else 'NOT BELOW'} (caller / bicgstab = {caller / bi:.3f})")
        print(f"{n}^3 f64: (c) bicgstab {bi:.4f} against cg x 21/11 = {cg * 21.0 / 11.0:.4f} (bicgstab / cg = {bi / cg:.3f}): reported")
        if "parent cg" in stat:
            par, pspread = stat["parent cg"]
            print(f"{n}^3 f64: (b) cg {cg:.4f} against the parent's {par:.4f}, margin {pspread:.4f}: "
                  f"{'within' if cg <= par + pspread else 'ABOVE'}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--mode", choices=["cg", "caller", "bicgstab"], default="bicgstab")
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
