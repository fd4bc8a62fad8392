#!/usr/bin/env python3
"""What multigrid on cell-centred grids costs next to the vertex-centred one, all alternated in one job, f64:

  1. the two transfer kernels alone on an N^3 fine field with every dimension halved (neptune_mg_restrict_cell,
     neptune_mg_prolong_add_cell) and, beside them, the vertex-centred kernels on (N - 1)^3, each against its pass model at
     the rate of a device-to-device copy of one fine field measured in the same process.  Pass models, in fine fields:
     restriction 2 read + 2 / 8 written, prolongation 1 read + 1 written + 1 / 8 read.  Reported: the fraction of the model's
     rate each kernel reaches; the claim looked at is that the cell-centred ones reach at least the vertex-centred ones'
     fraction, the margin being the spread (max - min) of the vertex-centred repetitions.
  2. ms per V(2,2) cycle of multigrid.solve and per multigrid.cg_solve iteration, and cycles / iterations to r . r <= 1e-16
     r0 . r0, on the N^3 cell-centred hierarchy (multigrid.coarsening_plan(..., centring="cell"), down to 2^3) and on the
     (N - 1)^3 vertex-centred one, per fine cell.  The vertex-centred levels run the unscaled 7-point star of
     examples/poisson_anisotropic_semicoarsening.py with weights 1 and a zero rim.  The cell-centred levels run the same star
     plus s u, s = the number of boundary faces of the cell in a second input field: the value 0 ON the faces (the ghost cell
     mirrored), one more field read per apply.  (The star alone would put the value 0 at the ghost cells' centres, a boundary
     that moves with the level: plain cycles diverge on it.)
  3. with --parent-tree: ms per cycle of multigrid.solve at (N - 1)^3 from this build against the PARENT commit's build (a
     checkout of it with its library built), the same tools/mgsemi_bench.py --kind cycle_full run from either tree side by side,
     repetition by repetition, the order of the two swapped every repetition.  The two
     must agree within the spread of the parent's own repetitions: the dispatch on the grid kind is host-side only.

  tools/mgcc_bench.py [--n 512] [--reps 3] [--cycles 10] [--limit SECONDS] [--parent-tree DIR] [--out profiles/mg_cellcentred.txt]
  tools/mgcc_bench.py --prefetch [--n 512]       compile every level's module into the module cache (no GPU)

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.

  --one --kind KIND --n N      one measurement (what a child runs); prints one JSON line.  KIND:
      transfer_cell / transfer_vertex    the copy and the two transfer kernels alone, device-event times
      cycle_cell / cycle_vertex          --cycles cycles of multigrid.solve with no tolerance, one warm-up run first
      iter_cell / iter_vertex            --cycles iterations of multigrid.cg_solve with no tolerance, one warm-up run first
      solve_cell / solve_vertex, cg_cell / cg_vertex    cycles / iterations to the tolerance"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
RTOL2 = 1e-16
KINDS = [f"{k}_{g}" for k in ("transfer", "cycle", "iter", "solve", "cg") for g in ("cell", "vertex")]


def _example():
    sys.path[:0] = [str(REPO / "neptune-pde-solver_amd"), str(REPO / "examples")]
    import poisson_anisotropic_semicoarsening as ex
    return ex


def plan_of(kind, n):
    """[(extents, weights, axes)]: the cell-centred plan on n^3, or full coarsening of the vertex-centred (n - 1)^3"""
    from neptune_hip import multigrid
    m = n if kind.endswith("cell") else n - 1
    return multigrid.coarsening_plan((m,) * 3, (1.0,) * 3, centring="cell" if kind.endswith("cell") else "vertex")


def cell_text(m):
    """@entry(out, u, s): out = (6 + s) u - (the six neighbours) on the interior m^3 of a box two cells larger per dimension"""
    import neptune as nep
    nep.reset()
    box = ([0, 0, 0], [m + 2] * 3)
    interior = ([1, 1, 1], [m + 1] * 3)
    c = nep.get_compiler()
    c.start_function("entry", [("memref", 3)] * 3)
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u, s = (nep.load(nep.wrap(nep.Expr(c.get_function_arg(1 + i)), box)) for i in range(2))

    @nep.apply(inputs=[u, s], bounds=interior)
    def star(x, d):
        return (x[0, 0, 0] * 6.0 - ((x[-1, 0, 0] + x[1, 0, 0]) + (x[0, -1, 0] + x[0, 1, 0]) + (x[0, 0, -1] + x[0, 0, 1]))) + d[0, 0, 0] * x[0, 0, 0]

    nep.store(star, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text, interior


def boundary_faces(m):
    """s over the (m + 2)^3 box: the number of boundary faces of each interior cell, 0 on the rim"""
    import numpy as np
    s = np.zeros((m + 2,) * 3)
    for d in range(3):
        for edge in (1, m):
            sl = [slice(1, m + 1)] * 3
            sl[d] = slice(edge, edge + 1)
            s[tuple(sl)] += 1.0
    return s


def cell_hierarchy(plan, ex):
    """one lowered operator per level of the cell-centred plan (every level a cube)"""
    import numpy as np
    from neptune_hip import fields, lowering, multigrid
    F = fields.DeviceField
    levels = []
    for l, (extents, _, _) in enumerate(plan):
        m = extents[0]
        text, interior = cell_text(m)
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        like = F.from_numpy(np.zeros((m + 2,) * 3))
        others = [F.from_numpy(boundary_faces(m))]
        minv = multigrid.jacobi_weights(entry, like, interior, others=others, omega=ex.OMEGA, reach=1)
        levels.append(multigrid.Level(entry, like, interior, others=others, minv=minv, rscale=4.0))
    h = multigrid.Hierarchy(levels)
    assert h.halved == [p[2] for p in plan[:-1]]
    return h


def prefetch(n):
    """every level's module of both hierarchies into the module cache, side by side; no GPU is touched"""
    from concurrent.futures import ThreadPoolExecutor
    ex = _example()
    from neptune_hip import lowering
    jobs = {}
    for l, (extents, weights, _) in enumerate(plan_of("cycle_vertex", n)):
        jobs[(ex.build_text(extents, weights)[0], l == 0)] = None
    for l, (extents, _, _) in enumerate(plan_of("cycle_cell", n)):
        jobs[(cell_text(extents[0])[0], l == 0)] = None
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda j: lowering.compile_module(j[0], load=False, dot_entries=j[1]), jobs))
    print(f"{len(jobs)} modules in {lowering.cache_dir()}")


def transfer(args, out):
    """the copy of one fine field and the two transfer kernels alone, every dimension halved / coarsened"""
    import torch
    from neptune_hip import _capi, fields, multigrid
    cell = args.kind.endswith("cell")
    m = args.n if cell else args.n - 1
    field = lambda shape: fields.DeviceField((0,) * 3, tuple(shape), _capi.F64, torch.rand(tuple(shape), dtype=torch.float64, device="cuda"))
    level = lambda ext: multigrid.Level(None, field([v + 2 for v in ext]), ([1] * 3, [v + 1 for v in ext]))
    fine = level((m,) * 3)
    ext = multigrid.coarsen_bounds(fine.bounds, centring="cell" if cell else "vertex")
    coarse = level(ext)
    assert multigrid.halved_axes(fine, coarse) == ((0, 1, 2) if cell else ())
    bf, qf, xf = (field([m + 2] * 3) for _ in range(3))
    bc, xc = field([v + 2 for v in ext]), field([v + 2 for v in ext])
    times = {}
    for name, launch in (("copy", lambda: qf.tensor.copy_(bf.tensor)),
                         ("restrict", lambda: multigrid.restrict(fine, coarse, bf, qf, bc, xc)),
                         ("prolong_add", lambda: multigrid.prolong_add(fine, coarse, xc, xf))):
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
    box, omega = float((m + 2) ** 3 * 8), float(m ** 3 * 8)
    rate = 2.0 * box / times["copy"]                       # bytes per ms: the copy reads and writes the whole box
    model = {"restrict": (2.0 + 2.0 / 8.0) * omega / rate, "prolong_add": (2.0 + 1.0 / 8.0) * omega / rate}
    out.update(m=m, launches=args.launches, copy_ms=times["copy"], copy_TBps=rate * 1e-9,
               restrict_ms=times["restrict"], prolong_ms=times["prolong_add"],
               restrict_fraction=model["restrict"] / times["restrict"], prolong_fraction=model["prolong_add"] / times["prolong_add"])


def one(args):
    ex = _example()
    import torch
    from neptune_hip import _capi, fields, multigrid
    _capi.load().neptune_hip_init(0)
    out = {"kind": args.kind, "n": args.n}
    if args.kind.startswith("transfer"):
        transfer(args, out)
        print(json.dumps(out))
        return
    F = fields.DeviceField
    plan = plan_of(args.kind, args.n)
    m = plan[0][0][0]
    h = cell_hierarchy(plan, ex) if args.kind.endswith("cell") else ex.hierarchy(plan)[0]
    b = F.from_numpy(ex.right_hand_side(m))
    x = F.empty_like(b)
    work = [F.empty_like(b) for _ in range(3)]
    out.update(m=m, levels=len(h), coarsest=list(plan[-1][0]))

    def timed(fn):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    K = args.cycles
    what = args.kind.split("_")[0]
    if what == "cycle":
        run = lambda: multigrid.solve(h, x, b, pre=ex.SWEEPS, post=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=K, tol2=0.0,
                                      check_every=K)
    elif what == "iter":
        run = lambda: multigrid.cg_solve(h, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=K, tol2=0.0, check_every=K,
                                         work=work)
    else:
        x.tensor.zero_()
        _, rr0, _ = multigrid.cg_solve(h, x, b, max_iters=0)
        tol2 = RTOL2 * rr0
        if what == "solve":
            run = lambda: multigrid.solve(h, x, b, pre=ex.SWEEPS, post=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=args.max_cycles,
                                          tol2=tol2, check_every=1)[:3]
        else:
            run = lambda: multigrid.cg_solve(h, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=ex.MAX_ITERS, tol2=tol2,
                                             work=work)
    timed(run)
    res, seconds = timed(run)
    if what in ("cycle", "iter"):
        out.update(steps=int(res[0]), ms_per_step=seconds * 1e3 / K, ns_per_cell=seconds * 1e9 / K / m ** 3)
    else:
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

    say(f"# tools/mgcc_bench.py --n {args.n} --reps {args.reps} --cycles {args.cycles}"
        + (" --parent-tree <a checkout of the parent commit>" if args.parent_tree else ""))
    common = ["--n", str(args.n), "--cycles", str(args.cycles)]
    jobs = [(k, [me, "--one", "--kind", k] + common) for k in KINDS if not k.startswith(("solve", "cg"))]
    pair = []
    if args.parent_tree:                           # the same tool from both trees, side by side
        for label, tree in (("this cycle_full", REPO), ("parent cycle_full", Path(args.parent_tree).resolve())):
            pair.append((label, [str(tree / "tools" / "mgsemi_bench.py"), "--one", "--kind", "cycle_full", "--m", str(args.n - 1),
                                 "--cycles", str(args.cycles)]))
    once = [(k, [me, "--one", "--kind", k] + common) for k in KINDS if k.startswith(("solve", "cg"))]
    for rep in range(args.reps):                   # the kinds alternate repetition by repetition; the pair swaps its order
        for label, cmd in jobs + (pair if rep % 2 == 0 else pair[::-1]) + (once if rep == 0 else []):
            if child(label, cmd) is None:
                _write(args, lines)
                return 1

    med = lambda label, key: statistics.median(r[key] for r in results[label])
    spread = lambda label, key: max(r[key] for r in results[label]) - min(r[key] for r in results[label])
    n = args.n
    say(f"1. transfer kernels alone, f64, {n}^3 halved onto {n // 2}^3 and {n - 1}^3 coarsened onto {(n - 2) // 2}^3; fraction of the pass "
        f"model's rate at the copy's rate of the same process (median of {args.reps}, spread = max - min):")
    for g in ("cell", "vertex"):
        lab = f"transfer_{g}"
        say(f"  {g:>6}: copy {med(lab, 'copy_TBps'):.2f} TB/s; restrict {med(lab, 'restrict_ms'):.3f} ms = {med(lab, 'restrict_fraction'):.3f} of "
            f"its model (spread {spread(lab, 'restrict_fraction'):.3f}); prolong_add {med(lab, 'prolong_ms'):.3f} ms = "
            f"{med(lab, 'prolong_fraction'):.3f} (spread {spread(lab, 'prolong_fraction'):.3f})")
    for key, name in (("restrict_fraction", "restrict"), ("prolong_fraction", "prolong_add")):
        c, v, margin = med("transfer_cell", key), med("transfer_vertex", key), spread("transfer_vertex", key)
        say(f"  {name}: cell / vertex fraction = {c:.3f} / {v:.3f} = {c / v:.2f}; cell >= vertex - its spread ({margin:.3f}): {c >= v - margin}")
    say(f"2. {n}^3 cell-centred ({results['cycle_cell'][0]['levels']} levels, coarsest {results['cycle_cell'][0]['coarsest']}) against "
        f"{n - 1}^3 vertex-centred ({results['cycle_vertex'][0]['levels']} levels), 7-point star (cell-centred: plus s u from a second field), V(2,2), 8 coarse sweeps:")
    for what, unit in (("cycle", "V(2,2) cycle"), ("iter", "cg_solve iteration")):
        c, v = f"{what}_cell", f"{what}_vertex"
        say(f"  ms per {unit}: cell {med(c, 'ms_per_step'):.3f} (spread {spread(c, 'ms_per_step'):.3f}), vertex {med(v, 'ms_per_step'):.3f} "
            f"(spread {spread(v, 'ms_per_step'):.3f}); ns per fine cell: {med(c, 'ns_per_cell'):.4f} / {med(v, 'ns_per_cell'):.4f} = "
            f"{med(c, 'ns_per_cell') / med(v, 'ns_per_cell'):.3f}")
    for what, unit in (("solve", "cycles"), ("cg", "iterations")):
        c, v = results[f"{what}_cell"][0], results[f"{what}_vertex"][0]
        say(f"  {unit} to r.r <= {RTOL2:g} r0.r0: cell {c['steps']} ({c['ms']:.1f} ms, reached: {c['reached']}, r.r / r0.r0 = "
            f"{c['rr_over_rr0']:.1e}), vertex {v['steps']} ({v['ms']:.1f} ms, reached: {v['reached']})")
    if args.parent_tree:
        a, p = med("this cycle_full", "ms_per_cycle"), med("parent cycle_full", "ms_per_cycle")
        margin = spread("parent cycle_full", "ms_per_cycle")
        say(f"3. ms per cycle of multigrid.solve at {n - 1}^3 (tools/mgsemi_bench.py --kind cycle_full from either tree), this build / the "
            f"parent's build: {a:.3f} / {p:.3f} = {a / p:.4f}; this build's repetitions {[round(r['ms_per_cycle'], 3) for r in results['this cycle_full']]}, "
            f"the parent's {[round(r['ms_per_cycle'], 3) for r in results['parent cycle_full']]}; the parent's spread {margin:.3f} ms; within it: "
            f"{abs(a - p) <= margin}")
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
    ap.add_argument("--kind", choices=KINDS, default="transfer_cell")
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
        prefetch(args.n)
        return 0
    if args.one:
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
