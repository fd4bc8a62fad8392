#!/usr/bin/env python3
"""What semi-coarsening buys on an axis-aligned anisotropic operator and what its transfer kernels cost, all
alternated in one job, on the problem of examples/poisson_anisotropic_semicoarsening.py (eps = 0.03 along dimension 0, f64,
V(2,2), 8 coarse sweeps):

  * cycles / iterations and wall time to r . r <= 1e-16 r0 . r0 for multigrid.solve and multigrid.cg_solve, each on the
    semi-coarsened hierarchy (multigrid.coarsening_plan) and on the fully coarsened one.  With --parent-tree the two
    full-coarsening solvers are ALSO timed from the PARENT commit's build (a checkout of it with its library built: its own
    tools/mgcg_bench.py is run there), repetition by repetition with this build's.  Margin: the spread (max - min) of each
    solver's own repetitions.
  * ms per cycle of multigrid.solve on both hierarchies (--cycles cycles, no tolerance) against the pass model; reported,
    not judged.
  * the two transfer kernels alone on a --transfer^3 fine field: time per byte of fine-field traffic (restriction: b and q
    read once; prolongation: x read and written) for each of the seven masks of coarsened dimensions, against the full mask,
    whose kernel is the parent's; reported, not judged.

  tools/mgsemi_bench.py [--sizes 127,255] [--reps 3] [--cycles 10] [--transfer 255] [--limit SECONDS] [--parent-tree DIR]
                        [--out profiles/mg_semicoarsen.txt]
  tools/mgsemi_bench.py --prefetch [--sizes ...]     compile every level's module into the module cache (no GPU)

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.

  --one --kind KIND --m M      one measurement (what a child runs); prints one JSON line.  KIND:
      solve_semi / solve_full / cg_semi / cg_full    cycles or iterations and wall time to the tolerance, one warm-up run first
      cycle_semi / cycle_full                        --cycles cycles of multigrid.solve with no tolerance, one warm-up run
      transfer                                       the two transfer kernels alone, every mask, device-event times"""
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
SOLVE_KINDS = ["solve_semi", "solve_full", "cg_full", "cg_semi"]
PARENT_KINDS = {"parent solve_full": "aniso_mg", "parent cg_full": "aniso_mgcg"}


def _example():
    sys.path[:0] = [str(REPO / "neptune-pde-solver_amd"), str(REPO / "examples")]
    import poisson_anisotropic_semicoarsening as ex
    return ex


def prefetch(sizes):
    """every level's module of both hierarchies of every size into the module cache, side by side; no GPU is touched"""
    from concurrent.futures import ThreadPoolExecutor
    ex = _example()
    from neptune_hip import lowering
    jobs = {}
    for m in sizes:
        for plan in (ex.semi_plan(m), ex.full_plan(m)):
            for l, (extents, weights, _) in enumerate(plan):
                jobs[(ex.build_text(extents, weights)[0], l == 0)] = None
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda j: lowering.compile_module(j[0], load=False, dot_entries=j[1]), jobs))
    print(f"{len(jobs)} modules in {lowering.cache_dir()}")


def transfer(args, out):
    """restriction and prolongation alone on an m^3 fine Omega, every mask of coarsened dimensions (bit d = dimension d)"""
    import torch
    from neptune_hip import _capi, fields, multigrid
    m = args.m
    f64 = torch.float64
    field = lambda shape: fields.DeviceField((0,) * 3, tuple(shape), _capi.F64, torch.rand(tuple(shape), dtype=f64, device="cuda"))
    level = lambda ext: multigrid.Level(None, field([v + 2 for v in ext]), ([1] * 3, [v + 1 for v in ext]))
    fine = level((m,) * 3)
    bf, qf, xf = (field([m + 2] * 3) for _ in range(3))
    fine_bytes = (m + 2) ** 3 * 8
    rows = {}
    for mask in range(1, 8):
        axes = tuple(d for d in range(3) if mask >> d & 1)
        ext = multigrid.coarsen_bounds(fine.bounds, axes=axes)
        coarse = level(ext)
        assert multigrid.coarsened_axes(fine, coarse) == axes
        bc, xc = field([v + 2 for v in ext]), field([v + 2 for v in ext])
        times = {}
        for name, launch in (("restrict", lambda: multigrid.restrict(fine, coarse, bf, qf, bc, xc)),
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
        rows["".join(str(mask >> d & 1) for d in range(3))] = {"coarse": list(ext), "restrict_ms": times["restrict"],
                                                                "prolong_ms": times["prolong_add"]}
    out.update(fine_bytes=fine_bytes, launches=args.launches, masks=rows)


def one(args):
    ex = _example()
    import torch
    from neptune_hip import _capi, fields, multigrid
    lib = _capi.load()
    lib.neptune_hip_init(0)
    out = {"kind": args.kind, "m": args.m}
    if args.kind == "transfer":
        transfer(args, out)
        print(json.dumps(out))
        return
    F = fields.DeviceField
    which = args.kind.split("_")[1]
    plan = ex.semi_plan(args.m) if which == "semi" else ex.full_plan(args.m)
    h = ex.hierarchy(plan)[0]
    b = F.from_numpy(ex.right_hand_side(args.m))
    x = F.empty_like(b)
    work = [F.empty_like(b) for _ in range(3)]
    out.update(levels=len(h), passes_per_cycle=ex.passes_per_cycle(plan, ex.SWEEPS, ex.SWEEPS),
               passes_per_iteration=ex.passes_per_iteration(plan))

    def timed(fn):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    if args.kind.startswith("cycle"):
        K = args.cycles
        run = lambda: multigrid.solve(h, x, b, pre=ex.SWEEPS, post=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=K, tol2=0.0,
                                      check_every=K)
        timed(run)
        res, seconds = timed(run)
        out.update(steps=int(res[0]), counts=list(multigrid.counts()), ms_per_cycle=seconds * 1e3 / K)
    else:
        x.tensor.zero_()
        _, rr0, _ = multigrid.cg_solve(h, x, b, max_iters=0)
        tol2 = RTOL2 * rr0
        if args.kind.startswith("solve"):
            run = lambda: multigrid.solve(h, x, b, pre=ex.SWEEPS, post=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=ex.MAX_CYCLES,
                                          tol2=tol2, check_every=1 if which == "semi" else 4)[:3]
        else:
            run = lambda: multigrid.cg_solve(h, x, b, sweeps=ex.SWEEPS, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=ex.MAX_ITERS, tol2=tol2,
                                             work=work)
        timed(run)
        res, seconds = timed(run)
        out.update(steps=int(res[0]), ms=seconds * 1e3, rr0=rr0, rr_last=res[2], reached=bool(res[2] <= tol2))
    print(json.dumps(out))


def drive(args):
    sizes = [int(s) for s in args.sizes.split(",") if s]
    lines, results = [], {}
    me = str(Path(__file__).resolve())

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def child(label, m, cmd):
        """one measurement in a fresh process under its own time limit; -> its JSON, or None after saying why"""
        p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            say(f"{label} m={m}: exit status {p.returncode}; nothing more is started")
            return None
        out = json.loads(p.stdout.strip().splitlines()[-1])
        out["label"] = label
        say(json.dumps(out))
        results.setdefault((m, label), []).append(out)
        return out

    def stop():
        _write(args, lines)
        return 1

    say(f"# tools/mgsemi_bench.py --sizes {args.sizes} --reps {args.reps} --cycles {args.cycles} --transfer {args.transfer}"
        + (" --parent-tree <a checkout of the parent commit>" if args.parent_tree else ""))
    jobs = [(k, [me, "--one", "--kind", k]) for k in SOLVE_KINDS]
    if args.parent_tree:
        parent = str(Path(args.parent_tree).resolve() / "tools" / "mgcg_bench.py")
        jobs += [(label, [parent, "--one", "--kind", kind]) for label, kind in PARENT_KINDS.items()]
    jobs += [(k, [me, "--one", "--kind", k, "--cycles", str(args.cycles)]) for k in ("cycle_semi", "cycle_full")]
    for m in sizes:
        for rep in range(args.reps):
            for label, cmd in jobs:
                if child(label, m, cmd + ["--m", str(m)]) is None:
                    return stop()
    if args.transfer:
        for rep in range(args.reps):
            if child("transfer", args.transfer, [me, "--one", "--kind", "transfer", "--m", str(args.transfer)]) is None:
                return stop()

    med = lambda m, label, key: statistics.median(r[key] for r in results[(m, label)])
    spread = lambda m, label, key: max(r[key] for r in results[(m, label)]) - min(r[key] for r in results[(m, label)])
    for m in sizes:
        say(f"{m}^3 f64, eps = 0.03 along dimension 0, V(2,2), 8 coarse sweeps, to r.r <= {RTOL2:g} r0.r0 "
            f"(levels: semi {results[(m, 'solve_semi')][0]['levels']}, full {results[(m, 'solve_full')][0]['levels']}):")
        for label in SOLVE_KINDS + (list(PARENT_KINDS) if args.parent_tree else []):
            rs = results[(m, label)]
            unit = "cycles" if "solve" in label else "iterations"
            say(f"  {label:>18}: {rs[0]['steps']} {unit}, {med(m, label, 'ms'):.1f} ms (spread {spread(m, label, 'ms'):.1f}), "
                f"reached: {all(r['reached'] for r in rs)}")
        if args.parent_tree:
            for label in PARENT_KINDS:
                mine = label.split()[1]
                a, p = med(m, mine, "ms"), med(m, label, "ms")
                say(f"  full coarsening, this build / the parent's build, {mine}: {a:.1f} / {p:.1f} = {a / p:.3f} "
                    f"(the parent's spread {spread(m, label, 'ms'):.1f} ms; the parent's tool draws its own right-hand side)")
        base = "parent cg_full" if args.parent_tree else "cg_full"
        best, semi = med(m, base, "ms"), med(m, "solve_semi", "ms")
        margin = spread(m, "solve_semi", "ms")
        say(f"  multigrid.solve on the semi-coarsened hierarchy against {base}: {best:.1f} / {semi:.1f} = {best / semi:.2f} "
            f"({'faster beyond its own spread' if semi + margin < best else 'NOT faster beyond its own spread'})")
        cs, cf = results[(m, "cycle_semi")][0], results[(m, "cycle_full")][0]
        ms_s, ms_f = med(m, "cycle_semi", "ms_per_cycle"), med(m, "cycle_full", "ms_per_cycle")
        say(f"  ms per cycle: semi {ms_s:.3f} (spread {spread(m, 'cycle_semi', 'ms_per_cycle'):.3f}), full {ms_f:.3f} "
            f"(spread {spread(m, 'cycle_full', 'ms_per_cycle'):.3f}): semi / full = {ms_s / ms_f:.3f} "
            f"(pass model {cs['passes_per_cycle']:.1f} / {cf['passes_per_cycle']:.1f} = {cs['passes_per_cycle'] / cf['passes_per_cycle']:.3f})")
    if args.transfer:
        m = args.transfer
        rs = results[(m, "transfer")]
        fine = rs[0]["fine_bytes"]
        say(f"transfer kernels alone, fine Omega {m}^3 f64 ({fine} bytes per fine field), mask = dimensions 0 1 2 coarsened; ps per byte "
            f"of fine-field traffic (2 fine fields each), median of {len(rs)} processes x {rs[0]['launches']} launches, and against mask 111:")
        ps = lambda key, mask: statistics.median(r["masks"][mask][key] for r in rs) * 1e9 / (2 * fine)
        for mask in sorted(rs[0]["masks"]):
            r, p = ps("restrict_ms", mask), ps("prolong_ms", mask)
            say(f"  mask {mask} (coarse {'x'.join(str(v) for v in rs[0]['masks'][mask]['coarse'])}): restrict {r:.3f} ps/B ({r / ps('restrict_ms', '111'):.2f}x), "
                f"prolong_add {p:.3f} ps/B ({p / ps('prolong_ms', '111'):.2f}x)")
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
    ap.add_argument("--kind", choices=SOLVE_KINDS + ["cycle_semi", "cycle_full", "transfer"], default="solve_semi")
    ap.add_argument("--m", type=int, default=127)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sizes", default="127,255")
    ap.add_argument("--transfer", type=int, default=255)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.prefetch:
        prefetch([int(s) for s in args.sizes.split(",") if s])
        return 0
    if args.one:
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
