#!/usr/bin/env python3
"""What the linear prolongation on cell-centred grids costs and buys, by the method of tools/mgcc_bench.py: every
measurement a fresh child process under its own time limit, the kinds alternated repetition by repetition, spread reported.

  1. the kernel alone, N^3 -> (N/2)^3, every dimension halved, f64 and f32 (neptune_mg_prolong_add_linear), in the same
     process as its two yardsticks: the constant kernel (neptune_mg_prolong_add_cell) and the pass model -- 1 fine field
     read + 1 written + 1 / 8 read -- at the rate of a device-to-device copy of one fine field; beside them the vertex-centred
     prolongation on (N - 1)^3.
  2. plain cycles on the N^3 Dirichlet-face hierarchy of tools/mgcc_bench.py (the star plus s u, down to 2^3), V(2,2):
     cycles and ms to r . r <= 1e-16 r0 . r0 with linear prolongation on every pair, beside multigrid.cg_solve on the same
     levels with the constant prolongation (conjugate gradients take no linear pair); ms per cycle, linear against constant.
  3. with --parent-tree: the paths this does not touch, ms per cycle of multigrid.solve with constant transfers at N^3
     (tools/mgcc_bench.py --kind cycle_cell) and vertex-centred at (N - 1)^3 (tools/mgsemi_bench.py --kind cycle_full), the same
     tool run from this tree and from a checkout of the PARENT commit with its library built, side by side, the order of the
     two swapped every repetition.  Each ratio must lie inside the spread of the parent's own repetitions.

  tools/mgcl_bench.py [--n 512] [--reps 3] [--cycles 10] [--limit SECONDS] [--parent-tree DIR] [--out profiles/mg_linear.txt]
  tools/mgcl_bench.py --prefetch [--n 512]       compile every level's module into the module cache (no GPU)

The driver touches no GPU; it checks every exit status and starts nothing more after a child that failed, was killed or ran
into its limit.

  --one --kind KIND --n N      one measurement (what a child runs); prints one JSON line.  KIND:
      transfer_f64 / transfer_f32       the copy and the prolongation kernels alone, device-event times
      cycle_linear / cycle_constant     --cycles cycles of multigrid.solve with no tolerance, one warm-up run first
      solve_linear / cg_constant        cycles / iterations to the tolerance"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path.insert(0, str(HERE))
import mgcc_bench as base     # noqa: E402  (the hierarchy, the operator and the prefetch of the cell-centred problem)

RTOL2 = base.RTOL2
KINDS = ["transfer_f64", "transfer_f32", "cycle_linear", "cycle_constant", "solve_linear", "cg_constant"]


def transfer(args, out):
    """the copy of one fine field, the constant and the linear prolongation on n^3 -> (n / 2)^3, and the
    vertex-centred prolongation on (n - 1)^3 -> ((n - 2) / 2)^3, all in this process"""
    import torch
    from neptune_hip import _capi, fields, multigrid
    wide = args.kind.endswith("f64")
    dtype, tdtype, size = (_capi.F64, torch.float64, 8) if wide else (_capi.F32, torch.float32, 4)
    n = args.n
    field = lambda shape: fields.DeviceField((0,) * 3, tuple(shape), dtype, torch.rand(tuple(shape), dtype=tdtype, device="cuda"))

    def pair(m, centring, **setting):
        level = lambda ext, **kw: multigrid.Level(None, field([v + 2 for v in ext]), ([1] * 3, [v + 1 for v in ext]), **kw)
        fine = level((m,) * 3, **setting)
        ext = multigrid.coarsen_bounds(fine.bounds, centring=centring)
        return fine, level(ext), field([v + 2 for v in ext]), field([m + 2] * 3)
    cell = pair(n, "cell")
    linear = (pair(n, "cell", prolong="linear", faces="dirichlet")[0],) + cell[1:]
    vertex = pair(n - 1, "vertex")
    src, dst = field([n + 2] * 3), field([n + 2] * 3)
    prolong = lambda p: (lambda: multigrid.prolong_add(p[0], p[1], p[2], p[3]))
    times = {}
    for name, launch in (("copy", lambda: dst.tensor.copy_(src.tensor)), ("constant", prolong(cell)), ("linear", prolong(linear)),
                         ("vertex", prolong(vertex))):
        for _ in range(3):
            launch()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.launches):
            launch()
        ev[1].record()
        torch.cuda.synchronize()
        times[name] = ev[0].elapsed_time(ev[1]) / args.launches
    rate = 2.0 * float((n + 2) ** 3 * size) / times["copy"]          # bytes per ms: the copy reads and writes the whole box
    model = lambda m: (2.0 + 1.0 / 8.0) * float(m ** 3 * size) / rate
    out.update(launches=args.launches, copy_ms=times["copy"], copy_TBps=rate * 1e-9)
    for name in ("constant", "linear", "vertex"):
        out[name + "_ms"] = times[name]
        out[name + "_fraction"] = model(n - 1 if name == "vertex" else n) / times[name]


def hierarchy(n, linear):
    """tools/mgcc_bench.py's cell-centred hierarchy on n^3 (the value 0 on every face); linear: every pair prolongs linearly"""
    ex = base._example()
    from neptune_hip import multigrid
    plan = base.plan_of("cycle_cell", n)
    levels = base.cell_hierarchy(plan, ex).levels
    if linear:
        for L in levels[:-1]:
            L.prolong, L.faces = "linear", "dirichlet"
    h = multigrid.Hierarchy(levels)
    assert h.has_linear == linear
    return ex, plan, h


def one(args):
    base._example()               # puts the package and the examples on the path
    import torch
    from neptune_hip import _capi, fields, multigrid
    _capi.load().neptune_hip_init(0)
    out = {"kind": args.kind, "n": args.n}
    if args.kind.startswith("transfer"):
        transfer(args, out)
        print(json.dumps(out))
        return
    F = fields.DeviceField
    ex, plan, h = hierarchy(args.n, args.kind.endswith("linear"))
    m = plan[0][0][0]
    b = F.from_numpy(ex.right_hand_side(m))
    x = F.empty_like(b)
    out.update(levels=len(h), coarsest=list(plan[-1][0]))

    def timed(fn):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    K = args.cycles
    sweeps = dict(pre=ex.SWEEPS, post=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS)
    if args.kind.startswith("cycle"):
        run = lambda: multigrid.solve(h, x, b, max_cycles=K, tol2=0.0, check_every=K, **sweeps)
    else:
        x.tensor.zero_()
        _, rr0, _, _ = multigrid.solve(h, x, b, max_cycles=0)
        tol2 = RTOL2 * rr0
        if args.kind == "solve_linear":
            run = lambda: multigrid.solve(h, x, b, max_cycles=args.max_cycles, tol2=tol2, check_every=1, **sweeps)
        else:
            work = [F.empty_like(b) for _ in range(3)]
            run = lambda: multigrid.cg_solve(h, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=ex.MAX_ITERS, tol2=tol2,
                                             work=work)
    timed(run)
    res, seconds = timed(run)
    if args.kind.startswith("cycle"):
        out.update(steps=int(res[0]), counts=list(multigrid.counts()), ms_per_step=seconds * 1e3 / K)
    else:
        out.update(steps=int(res[0]), ms=seconds * 1e3, reached=bool(res[2] <= tol2), rr_over_rr0=res[2] / rr0)
        if args.kind == "solve_linear":
            out["factors"] = [round(a / c, 2) for a, c in zip([rr0] + res[3], res[3])]
    print(json.dumps(out))


def drive(args):
    lines, results = [], {}
    me = str(Path(__file__).resolve())

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def child(label, cmd):
        """one measurement in a fresh process under its own time limit; -> its JSON, or None after saying why"""
        p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            say(f"{label}: exit status {p.returncode}; nothing more is started")
            return None
        out = json.loads(p.stdout.strip().splitlines()[-1])
        out["label"] = label
        say(json.dumps(out))
        results.setdefault(label, []).append(out)
        return out

    n = args.n
    say(f"# tools/mgcl_bench.py --n {n} --reps {args.reps} --cycles {args.cycles}"
        + (" --parent-tree <a checkout of the parent commit>" if args.parent_tree else ""))
    common = ["--n", str(n), "--cycles", str(args.cycles)]
    jobs = [(k, [me, "--one", "--kind", k] + common) for k in KINDS if k.startswith(("transfer", "cycle"))]
    once = [(k, [me, "--one", "--kind", k] + common) for k in KINDS if k.startswith(("solve", "cg"))]
    pairs = []
    if args.parent_tree:                           # the same tool from both trees, side by side
        for what, tool, extra in (("cycle_cell", "mgcc_bench.py", ["--kind", "cycle_cell", "--n", str(n)]),
                                  ("cycle_full", "mgsemi_bench.py", ["--kind", "cycle_full", "--m", str(n - 1)])):
            pairs.append([(f"{who} {what}", [str(tree / "tools" / tool), "--one"] + extra + ["--cycles", str(args.cycles)])
                          for who, tree in (("this", REPO), ("parent", Path(args.parent_tree).resolve()))])
    for rep in range(args.reps):                   # the kinds alternate repetition by repetition; each pair swaps its order
        untouched = [job for pair in pairs for job in (pair if rep % 2 == 0 else pair[::-1])]
        for label, cmd in jobs + untouched + (once if rep == 0 else []):
            if child(label, cmd) is None:
                _write(args, lines)
                return 1

    med = lambda label, key: statistics.median(r[key] for r in results[label])
    spread = lambda label, key: max(r[key] for r in results[label]) - min(r[key] for r in results[label])
    say(f"1. prolongation kernels alone, {n}^3 <- {n // 2}^3 (vertex: {n - 1}^3 <- {(n - 2) // 2}^3); ms, and the fraction of the pass model's "
        f"rate (2 + 1/8 fine fields) at the copy's rate of the same process (median of {args.reps}, spread = max - min):")
    for t in ("f64", "f32"):
        lab = f"transfer_{t}"
        say(f"  {t}: copy {med(lab, 'copy_TBps'):.2f} TB/s; " + "; ".join(
            f"{name} {med(lab, name + '_ms'):.3f} ms = {med(lab, name + '_fraction'):.3f} (spread {spread(lab, name + '_fraction'):.3f})"
            for name in ("constant", "linear", "vertex")))
        say(f"  {t}: linear / constant = {med(lab, 'linear_ms') / med(lab, 'constant_ms'):.3f}; linear's fraction >= the vertex-centred "
            f"one's - its spread ({spread(lab, 'vertex_fraction'):.3f}): "
            f"{med(lab, 'linear_fraction') >= med(lab, 'vertex_fraction') - spread(lab, 'vertex_fraction')}")
    s, g = results["solve_linear"][0], results["cg_constant"][0]
    say(f"2. {n}^3, the value 0 on every face ({s['levels']} levels, coarsest {s['coarsest']}), V(2,2), 8 coarse sweeps:")
    say(f"  plain cycles with linear prolongation to r.r <= {RTOL2:g} r0.r0: {s['steps']} cycles, {s['ms']:.1f} ms (reached: {s['reached']}, "
        f"r.r / r0.r0 = {s['rr_over_rr0']:.1e}); r.r factor per cycle: {s['factors']}")
    say(f"  cg_solve on the same levels with constant prolongation: {g['steps']} iterations, {g['ms']:.1f} ms (reached: {g['reached']}, "
        f"r.r / r0.r0 = {g['rr_over_rr0']:.1e}); plain cycles / cg_solve = {s['ms'] / g['ms']:.3f} in time")
    a, c = med("cycle_linear", "ms_per_step"), med("cycle_constant", "ms_per_step")
    say(f"  ms per V(2,2) cycle: linear {a:.3f} (spread {spread('cycle_linear', 'ms_per_step'):.3f}), constant {c:.3f} "
        f"(spread {spread('cycle_constant', 'ms_per_step'):.3f}); linear / constant = {a / c:.4f}")
    for pair, key, title in zip(pairs, ("ms_per_step", "ms_per_cycle"), (f"constant transfers at {n}^3 (tools/mgcc_bench.py --kind cycle_cell)",
                                                                         f"vertex-centred at {n - 1}^3 (tools/mgsemi_bench.py --kind cycle_full)")):
        this, parent = pair[0][0], pair[1][0]
        a, p, margin = med(this, key), med(parent, key), spread(parent, key)
        say(f"3. ms per cycle of multigrid.solve, {title}, this build / the parent's build: {a:.3f} / {p:.3f} = {a / p:.4f}; this build's "
            f"repetitions {[round(r[key], 3) for r in results[this]]}, the parent's {[round(r[key], 3) for r in results[parent]]}; the parent's "
            f"spread {margin:.3f} ms; within it: {abs(a - p) <= margin}")
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
    ap.add_argument("--kind", choices=KINDS, default="transfer_f64")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--max-cycles", type=int, default=60, help="the cap of the plain-cycle solve to the tolerance")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.prefetch:
        base.prefetch(args.n)
        return 0
    if args.one:
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
