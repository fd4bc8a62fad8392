#!/usr/bin/env python3
"""What the transposed linear restriction on cell-centred grids costs and buys, by the method of
tools/mgcl_bench.py: every measurement a fresh child process under its own time limit, the kinds alternated repetition by
repetition, spread reported.

  1. the kernel alone, f64, N^3 -> (N/2)^3 with every dimension halved and N^3 -> (N/2)^2 x N with the contiguous dimension
     kept (neptune_mg_restrict_linear), in the same process as its two yardsticks: the averaging kernel
     (neptune_mg_restrict_cell) on the same pair and the pass model -- 2 fine fields read + 2 coarse fields written -- at the
     rate of a device-to-device copy of one fine field.
  2. the N^3 Dirichlet-face hierarchy of tools/mgcc_bench.py (the star plus s u, down to 2^3), 8 coarse sweeps: iterations
     and ms to r . r <= 1e-16 r0 . r0 for multigrid.cg_solve on the symmetric linear pair at V(1,1) and V(2,2), beside
     cg_solve on the constant pair at V(2,2) and multigrid.solve on the linear / averaging pair of DESIGN 3.22 at V(2,2).
  3. with --parent-tree: the paths this does not touch, ms per cycle of multigrid.solve and ms per iteration of
     multigrid.cg_solve on the constant-pair hierarchy at N^3 (tools/mgcc_bench.py --kind cycle_cell / iter_cell), the same tool
     run from this tree and from a checkout of the PARENT commit with its library built, side by side, the order of the two
     swapped every repetition.  Each difference must lie inside the spread of the parent's own repetitions.

  tools/mgcs_bench.py [--n 512] [--reps 3] [--cycles 10] [--limit SECONDS] [--parent-tree DIR] [--out profiles/mg_symmetric.txt]
  tools/mgcs_bench.py --prefetch [--n 512]       compile every level's module into the module cache (no GPU)
  tools/mgcs_bench.py --one --kind transfer --n N --launches 1     what a counter run (rocprofv3 --pmc FETCH_SIZE) wraps

The driver touches no GPU; it checks every exit status and starts nothing more after a child that failed, was killed or ran
into its limit.

  --one --kind KIND --n N      one measurement (what a child runs); prints one JSON line.  KIND:
      transfer                                          the copy and the restriction kernels alone, device-event times
      cg_symmetric_v11 / cg_symmetric_v22 / cg_constant_v22 / solve_linear_average     iterations / cycles to the tolerance"""
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
SOLVES = ["cg_symmetric_v11", "cg_symmetric_v22", "cg_constant_v22", "solve_linear_average"]
KINDS = ["transfer"] + SOLVES
PAIRS = {"all": (0, 1, 2), "kept": (0, 1)}       # the dimensions halved: every one, or the contiguous one kept


def fine_bytes(n, axes, size=8):
    """the pass model of a restriction on n^3: (bytes that must be fetched, bytes that must be written)"""
    coarse = n ** 3 // 2 ** len(axes)
    return 2.0 * n ** 3 * size, 2.0 * coarse * size


def transfer(args, out):
    """the copy of one fine field, the averaging and the transposed linear restriction, on both pairs, all in this process"""
    import torch
    from neptune_hip import _capi, fields, multigrid
    n = args.n
    field = lambda shape: fields.DeviceField((0,) * 3, tuple(shape), _capi.F64, torch.rand(tuple(shape), dtype=torch.float64, device="cuda"))
    level = lambda ext, **kw: multigrid.Level(None, field([v + 2 for v in ext]), ([1] * 3, [v + 1 for v in ext]), **kw)
    bf, qf, src = (field([n + 2] * 3) for _ in range(3))
    launches = {"copy": lambda: src.tensor.copy_(bf.tensor)}
    for name, axes in PAIRS.items():
        ext = multigrid.coarsen_bounds(([1] * 3, [n + 1] * 3), axes=axes, centring="cell")
        coarse, bc, xc = level(ext), field([v + 2 for v in ext]), field([v + 2 for v in ext])
        for kind, setting in (("average", {}), ("linear", dict(restrict="linear", faces="dirichlet"))):
            fine = level((n,) * 3, **setting)
            assert multigrid.halved_axes(fine, coarse) == axes
            launches[f"{kind}_{name}"] = (lambda f=fine, c=coarse, b=bc, x=xc: multigrid.restrict(f, c, bf, qf, b, x))
    times = {}
    for name, launch in launches.items():
        for _ in range(min(3, args.launches)):
            launch()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.launches):
            launch()
        ev[1].record()
        torch.cuda.synchronize()
        times[name] = ev[0].elapsed_time(ev[1]) / args.launches
    rate = 2.0 * float((n + 2) ** 3 * 8) / times["copy"]          # bytes per ms: the copy reads and writes the whole box
    out.update(launches=args.launches, copy_ms=times["copy"], copy_TBps=rate * 1e-9)
    for name, axes in PAIRS.items():
        model = sum(fine_bytes(n, axes)) / rate
        for kind in ("average", "linear"):
            out[f"{kind}_{name}_ms"] = times[f"{kind}_{name}"]
            out[f"{kind}_{name}_fraction"] = model / times[f"{kind}_{name}"]


def hierarchy(n, prolong, restrict):
    """tools/mgcc_bench.py's cell-centred hierarchy on n^3 (the value 0 on every face), every pair with the two transfers"""
    ex = base._example()
    from neptune_hip import multigrid
    plan = base.plan_of("cycle_cell", n)
    levels = base.cell_hierarchy(plan, ex).levels
    for L in levels[:-1]:
        L.prolong, L.restrict, L.faces = prolong, restrict, "dirichlet"
    h = multigrid.Hierarchy(levels)
    assert h.has_linear == (prolong == "linear") and h.has_linear_restrict == (restrict == "linear")
    return ex, plan, h


def one(args):
    base._example()               # puts the package and the examples on the path
    import torch
    from neptune_hip import _capi, fields, multigrid
    _capi.load().neptune_hip_init(0)
    out = {"kind": args.kind, "n": args.n}
    if args.kind == "transfer":
        transfer(args, out)
        print(json.dumps(out))
        return
    F = fields.DeviceField
    form, pair, rest = args.kind.split("_", 2)
    prolong, restrict = {"symmetric": ("linear", "linear"), "constant": ("constant", "average"), "linear": ("linear", "average")}[pair]
    ex, plan, h = hierarchy(args.n, prolong, restrict)
    sweeps = 1 if rest == "v11" else ex.SWEEPS
    m = plan[0][0][0]
    b = F.from_numpy(ex.right_hand_side(m))
    x = F.empty_like(b)
    work = [F.empty_like(b) for _ in range(3)]
    out.update(levels=len(h), coarsest=list(plan[-1][0]), sweeps=sweeps, symmetric=h.symmetric)

    def timed(fn):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    x.tensor.zero_()
    _, rr0, _, _ = multigrid.solve(h, x, b, max_cycles=0)
    tol2 = RTOL2 * rr0
    if form == "solve":
        run = lambda: multigrid.solve(h, x, b, pre=sweeps, post=sweeps, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=args.max_cycles, tol2=tol2,
                                      check_every=1)[:3]
    else:
        run = lambda: multigrid.cg_solve(h, x, b, sweeps=sweeps, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=ex.MAX_ITERS, tol2=tol2, work=work)
    timed(run)
    res, seconds = timed(run)
    out.update(steps=int(res[0]), ms=seconds * 1e3, reached=bool(res[2] <= tol2), rr_over_rr0=res[2] / rr0)
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
    say(f"# tools/mgcs_bench.py --n {n} --reps {args.reps} --cycles {args.cycles}"
        + (" --parent-tree <a checkout of the parent commit>" if args.parent_tree else ""))
    jobs = [(k, [me, "--one", "--kind", k, "--n", str(n)]) for k in KINDS]
    pairs = []
    if args.parent_tree:                           # the same tool from both trees, side by side
        for what in ("cycle_cell", "iter_cell"):
            pairs.append([(f"{who} {what}", [str(tree / "tools" / "mgcc_bench.py"), "--one", "--kind", what, "--n", str(n), "--cycles",
                                             str(args.cycles)])
                          for who, tree in (("this", REPO), ("parent", Path(args.parent_tree).resolve()))])
    for rep in range(args.reps):                   # the kinds alternate repetition by repetition; each pair swaps its order
        untouched = [job for pair in pairs for job in (pair if rep % 2 == 0 else pair[::-1])]
        for label, cmd in jobs + untouched:
            if child(label, cmd) is None:
                _write(args, lines)
                return 1

    med = lambda label, key: statistics.median(r[key] for r in results[label])
    spread = lambda label, key: max(r[key] for r in results[label]) - min(r[key] for r in results[label])
    say(f"1. restriction kernels alone, f64, {n}^3 fine; ms, and the fraction of the pass model's rate (2 fine fields read + 2 coarse fields "
        f"written) at the copy's rate of the same process (median of {args.reps}, spread = max - min); copy {med('transfer', 'copy_TBps'):.2f} TB/s:")
    for name, title in (("all", f"-> {n // 2}^3, every dimension halved"), ("kept", f"-> {n // 2}^2 x {n}, the contiguous dimension kept")):
        say(f"  {title}: " + "; ".join(
            f"{kind} {med('transfer', f'{kind}_{name}_ms'):.3f} ms = {med('transfer', f'{kind}_{name}_fraction'):.3f} "
            f"(spread {spread('transfer', f'{kind}_{name}_fraction'):.3f})" for kind in ("average", "linear"))
            + f"; linear / average = {med('transfer', f'linear_{name}_ms') / med('transfer', f'average_{name}_ms'):.3f}")
    first = results[SOLVES[0]][0]
    say(f"2. {n}^3, the value 0 on every face ({first['levels']} levels, coarsest {first['coarsest']}), 8 coarse sweeps, to r.r <= {RTOL2:g} r0.r0 "
        f"(median of {args.reps} ms, spread = max - min):")
    titles = {"cg_symmetric_v11": "cg_solve, symmetric linear pair, V(1,1)", "cg_symmetric_v22": "cg_solve, symmetric linear pair, V(2,2)",
              "cg_constant_v22": "cg_solve, constant / averaging pair, V(2,2)", "solve_linear_average": "solve, linear / averaging pair, V(2,2)"}
    for k in SOLVES:
        r = results[k]
        say(f"  {titles[k]}: {sorted({v['steps'] for v in r})} steps, {med(k, 'ms'):.1f} ms (spread {spread(k, 'ms'):.1f}; reached: "
            f"{all(v['reached'] for v in r)}; r.r / r0.r0 = {r[0]['rr_over_rr0']:.1e})")
    best = min(SOLVES, key=lambda k: med(k, "ms"))
    say(f"  the fastest: {titles[best]}")
    for pair, what in zip(pairs, ("cycle of multigrid.solve", "iteration of multigrid.cg_solve")):
        this, parent = pair[0][0], pair[1][0]
        a, p, margin = med(this, "ms_per_step"), med(parent, "ms_per_step"), spread(parent, "ms_per_step")
        say(f"3. ms per {what}, constant transfers at {n}^3 (tools/mgcc_bench.py), this build / the parent's build: {a:.3f} / {p:.3f} = "
            f"{a / p:.4f}; this build's repetitions {[round(r['ms_per_step'], 3) for r in results[this]]}, the parent's "
            f"{[round(r['ms_per_step'], 3) for r in results[parent]]}; the parent's spread {margin:.3f} ms; within it: {abs(a - p) <= margin}")
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
    ap.add_argument("--kind", choices=KINDS, default="transfer")
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
