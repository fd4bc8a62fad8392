#!/usr/bin/env python3
"""What an f32 V-cycle inside f64 conjugate gradients buys (multigrid.cg_solve_mixed) against the all-f64
multigrid.cg_solve on the same problem, same machine, same job; reported, not judged.  The operator is the one of
examples/poisson_mixed_precision_mgcg.py at m^3, isotropic (eps = 1) and anisotropic (eps = 0.03), V(2, 2), 8 coarse sweeps:

  * time per iteration of both solvers (a fixed number of iterations, no tolerance; wall clock around the blocking call, a
    warm-up call first), the two alternated --reps times in one process;
  * iterations of both solvers to r . r <= 1e-16 r0 . r0 and to 1e-24 r0 . r0;
  * with --kernels M: the kernel times of one mixed run under `rocprofv3 --kernel-trace --stats` (a run of its own, plain
    launches) for the three kernels at the seam of the two precisions, against their pass models at the rate of a
    device-to-device copy of one f64 field measured in an unprofiled process:
        neptune_mgcg_update_mixed     reads p, q, x, r (f64), minv (f32); writes x, r (f64), r32, z32 (f32): 7.5 f64 passes
        neptune_mgcg_direction_mixed  reads z32 (f32), p (f64); writes p: 2.5 f64 passes
        neptune_mg_smooth_dot_wide    reads q, b, minv, x (f32); writes x: 2.5 f64 passes

  tools/mgcgmixed_bench.py [--sizes 255,511] [--eps 1.0,0.03] [--iters 10] [--reps 3] [--kernels 511] [--limit SECONDS]
                           [--out profiles/mgcg_mixed.txt]
  tools/mgcgmixed_bench.py --prefetch [--sizes ...] [--eps ...]     compile every module into the module cache (no GPU)

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.

  --one --kind KIND --m M --eps EPS     one measurement (what a child runs); prints one JSON line.  KIND:
      iter        both solvers, --iters iterations each, alternated --reps times in the one process: ms per iteration
      count       both solvers: iterations and wall time to 1e-16 and to 1e-24 r0 . r0
      copy        a device-to-device copy of one (m + 2)^3 f64 field, device-event time
      profiled    the mixed solver alone, --iters iterations twice, for the profiler (which sets NEPTUNE_HIP_MG_GRAPH=0)"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
KINDS = ["iter", "count", "copy", "profiled"]
SEAM = {"neptune_mgcg_update_mixed": 7.5, "neptune_mgcg_direction_mixed": 2.5, "neptune_mg_smooth_dot_wide": 2.5}
MAX_ITERS = 200


def _example():
    sys.path[:0] = [str(REPO / "neptune-pde-solver_amd"), str(REPO / "examples")]
    import poisson_mixed_precision_mgcg as ex
    return ex


def prefetch(sizes, epss):
    """every level's module of every size, weight and element type into the module cache, side by side; no GPU is touched"""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    ex = _example()
    from neptune_hip import lowering
    jobs = {}
    for m in sizes:
        for eps in epss:
            for l, ml in enumerate(ex.level_extents(m)):
                jobs[(ex.build_text(ml, np.float64, eps)[0], l == 0)] = None
                jobs[(ex.build_text(ml, np.float32, eps)[0], False)] = None
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda j: lowering.compile_module(j[0], load=False, dot_entries=j[1]), jobs))
    print(f"{len(jobs)} modules in {lowering.cache_dir()}")


def one(args):
    import numpy as np
    import torch
    ex = _example()
    from neptune_hip import _capi, fields, multigrid
    _capi.load().neptune_hip_init(0)
    F = fields.DeviceField
    m, eps = args.m, args.eps
    out = {"kind": args.kind, "m": m, "eps": eps}
    n = m + 2
    if args.kind == "copy":
        a, b = (torch.rand((n,) * 3, dtype=torch.float64, device="cuda") for _ in range(2))
        for _ in range(3):
            a.copy_(b)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(20):
            a.copy_(b)
        ev[1].record()
        torch.cuda.synchronize()
        out.update(field_bytes=n ** 3 * 8, ms=ev[0].elapsed_time(ev[1]) / 20)
        print(json.dumps(out))
        return
    b = F.from_numpy(ex.right_hand_side(m))
    x = F.empty_like(b)
    work = [F.empty_like(b) for _ in range(3)]
    solvers = {}
    if args.kind != "profiled":
        h = ex.hierarchy(m, np.float64, eps)[0]
        solvers["f64"] = lambda max_iters, tol2: multigrid.cg_solve(h, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS,
                                                                    max_iters=max_iters, tol2=tol2, work=work)
    outer, inner = ex.outer_level(m, eps)[0], ex.hierarchy(m, np.float32, eps)[0]
    solvers["mixed"] = lambda max_iters, tol2: multigrid.cg_solve_mixed(outer, inner, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS,
                                                                        max_iters=max_iters, tol2=tol2, work=work)

    def timed(name, max_iters, tol2):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solvers[name](max_iters, tol2)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    out["levels"] = len(inner)
    if args.kind == "count":
        for name in solvers:
            (_, rr0, _), _ = timed(name, 0, 0.0)
            out[name] = {}
            for label, rtol2 in (("to_1e-16", 1e-16), ("to_1e-24", 1e-24)):
                (done, _, rr_last), seconds = timed(name, MAX_ITERS, rtol2 * rr0)
                out[name][label] = {"iterations": int(done), "reached": bool(rr_last <= rtol2 * rr0), "rr_over_rr0": rr_last / rr0,
                                    "ms": seconds * 1e3}
    else:
        for name in solvers:
            timed(name, args.iters, 0.0)              # warm-up: first-use tuning, workspace growth
        out.update(iters=args.iters, ms_per_iteration={name: [] for name in solvers})
        for _ in range(args.reps):                    # the two solvers alternated
            for name in solvers:
                (done, _, _), seconds = timed(name, args.iters, 0.0)
                assert done == args.iters
                out["ms_per_iteration"][name].append(seconds * 1e3 / args.iters)
        out["launches"] = multigrid.cg_counts()
    print(json.dumps(out))


def kernel_stats(args, say, me, m, eps):
    """one mixed run under the profiler, in a run of its own; -> {kernel: average ms} for the seam kernels, or None"""
    env = dict(os.environ, NEPTUNE_HIP_MG_GRAPH="0")
    with tempfile.TemporaryDirectory(prefix="mgcgmixed_prof_") as raw:      # the profiler's files: read here, then dropped
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--",
               sys.executable, me, "--one", "--kind", "profiled", "--m", str(m), "--eps", str(eps), "--iters", str(args.iters)]
        p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=raw)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            say(f"profiled m={m}: exit status {p.returncode}; nothing more is started")
            return None
        found = {}
        for f in Path(raw).rglob("*kernel_stats.csv"):
            for row in csv.DictReader(open(f)):
                for name in SEAM:
                    if name in row["Name"] and "Lb1ELb1E" not in row["Name"] and "true, true>" not in row["Name"]:   # not the set-up's p = widen(z32)
                        calls, total = found.get(name, (0, 0.0))
                        found[name] = (calls + int(row["Calls"]), total + int(row["Calls"]) * float(row["AverageNs"]))
    return {k: (c, t / c / 1e6) for k, (c, t) in found.items() if c}


def drive(args):
    ints = lambda s: [int(v) for v in s.split(",") if v]
    floats = lambda s: [float(v) for v in s.split(",") if v]
    lines, results = [], {}
    me = str(Path(__file__).resolve())

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def child(kind, m, eps):
        """one measurement in a fresh process under its own time limit; -> its JSON, or None after saying why"""
        cmd = [me, "--one", "--kind", kind, "--m", str(m), "--eps", str(eps), "--iters", str(args.iters), "--reps", str(args.reps)]
        p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            say(f"{kind} m={m} eps={eps}: exit status {p.returncode}; nothing more is started")
            return None
        out = json.loads(p.stdout.strip().splitlines()[-1])
        say(json.dumps(out))
        results.setdefault((kind, m, eps), []).append(out)
        return out

    def stop():
        _write(args, lines)
        return 1

    sizes, epss = ints(args.sizes), floats(args.eps)
    say(f"# tools/mgcgmixed_bench.py --sizes {args.sizes} --eps {args.eps} --iters {args.iters} --reps {args.reps} --kernels {args.kernels}")
    for m in sizes:
        for eps in epss:
            for kind in ("iter", "count"):
                if child(kind, m, eps) is None:
                    return stop()
    stats = None
    if args.kernels:
        if child("copy", args.kernels, epss[0]) is None:
            return stop()
        stats = kernel_stats(args, say, me, args.kernels, epss[0])
        if stats is None:
            return stop()

    for m in sizes:
        for eps in epss:
            it, cn = results[("iter", m, eps)][0], results[("count", m, eps)][0]
            f, x = it["ms_per_iteration"]["f64"], it["ms_per_iteration"]["mixed"]
            mf, mx = statistics.median(f), statistics.median(x)
            say(f"{m}^3, eps = {eps:g}, {it['levels']} levels, V(2,2), median of {len(f)} alternated runs x {args.iters} iterations: all-f64 "
                f"{mf:.3f} ms per iteration (spread {max(f) - min(f):.3f}), mixed {mx:.3f} (spread {max(x) - min(x):.3f}): mixed / f64 = "
                f"{mx / mf:.3f}, f64 / mixed = {mf / mx:.2f}x")
            for name in ("to_1e-16", "to_1e-24"):
                a, b = cn["f64"][name], cn["mixed"][name]
                flag = lambda r: "" if r["reached"] else f" (NOT reached: r.r / r0.r0 = {r['rr_over_rr0']:.1e})"
                say(f"    {name} r0.r0: all-f64 {a['iterations']} iterations, {a['ms']:.1f} ms{flag(a)}; mixed {b['iterations']} iterations, "
                    f"{b['ms']:.1f} ms{flag(b)}")
    if stats is not None:
        c = results[("copy", args.kernels, epss[0])][0]
        rate = 2 * c["field_bytes"] / (c["ms"] * 1e-3)
        say(f"{args.kernels}^3: a copy of one f64 field ({c['field_bytes']} bytes) {c['ms']:.3f} ms = {rate / 1e12:.2f} TB/s; kernel times of one "
            f"profiled mixed run (rocprofv3 --kernel-trace --stats, plain launches):")
        for name, passes in SEAM.items():
            if name not in stats:
                say(f"    {name}: not in the trace")
                continue
            calls, ms = stats[name]
            model = passes * c["field_bytes"] / rate * 1e3
            say(f"    {name}: {calls} calls, {ms:.3f} ms on average; {passes} f64 passes at the copy's rate: {model:.3f} ms; measured / model = "
                f"{ms / model:.2f}")
    _write(args, lines)
    return 0


def _write(args, lines):
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--prefetch", action="store_true")
    ap.add_argument("--kind", choices=KINDS, default="iter")
    ap.add_argument("--m", type=int, default=255)
    ap.add_argument("--eps", default="1.0,0.03")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", default="255,511")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=511)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.prefetch:
        prefetch([int(s) for s in args.sizes.split(",") if s], [float(s) for s in args.eps.split(",") if s])
        return 0
    if args.one:
        args.eps = float(args.eps.split(",")[0])
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
