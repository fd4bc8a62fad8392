#!/usr/bin/env python3
"""What the two further forms of the line stage's kernel cost against the launches they replace, and what conjugate gradients
around a line-smoothed V-cycle buy, all alternated in one job; f64; reported, not judged:

  * on one m^3 field (--stage-sizes) along each axis: the apply-free stage (neptune_hip_mg_line_first) against the built-in
    7-point apply followed by the plain stage, and the stage with a sum (neptune_hip_mg_line_smooth_dot) against the plain
    stage followed by neptune_hip_dot; a device-to-device copy of one field in the same process gives the rate the pass
    models are held against (7 against 2 + 8 passes; 9 against 8 + 2).
  * on the operator of examples/poisson_varying_anisotropy_mgcg.py at m^2 (--sizes): iterations / cycles and wall time to
    r . r <= 1e-16 r0 . r0 for multigrid.cg_solve(lines=True) V(1,1) and V(2,2), multigrid.solve with the same stages, and
    multigrid.cg_solve around point Jacobi.
  * with --parent-tree (a checkout of the PARENT commit with its library built): multigrid.cg_solve on a hierarchy WITHOUT
    stages at --nostage^3 -- tools/mgcg_bench.py's `iteration`, run from this tree and from the parent's, repetition by
    repetition.  The ratio must sit inside the spread of the parent's own repetitions.

  tools/mgcglines_bench.py [--stage-sizes 255,511] [--sizes 1023,2047] [--nostage 255] [--reps 3] [--limit SECONDS]
                           [--parent-tree DIR] [--out profiles/mgcg_lines.txt]
  tools/mgcglines_bench.py --prefetch [--sizes ...]     compile every level's module into the module cache (no GPU)

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.

  --one --kind KIND --m M      one measurement (what a child runs); prints one JSON line.  KIND:
      stage                                                  the kernels alone on an m^3 field, device-event times
      cg_lines11 / cg_lines22 / solve_lines / cg_point       steps and wall time to the tolerance, one warm-up run first"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
RTOL2 = 1e-16
SOLVE_KINDS = ["cg_lines11", "cg_lines22", "solve_lines", "cg_point"]


def _example():
    sys.path[:0] = [str(REPO / "neptune-pde-solver_amd"), str(REPO / "examples")]
    import poisson_varying_anisotropy_lines as ex
    return ex


def prefetch(sizes):
    """every level's module of every size into the module cache, side by side; no GPU is touched"""
    from concurrent.futures import ThreadPoolExecutor
    ex = _example()
    from neptune_hip import lowering
    jobs = {}
    for m in sizes:
        for l, (a, _) in enumerate(ex.coefficients(m)):
            jobs[(ex.build_text(a.shape[0])[0], l == 0)] = None
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda j: lowering.compile_module(j[0], load=False, dot_entries=j[1]), jobs))
    print(f"{len(jobs)} modules in {lowering.cache_dir()}")


def stage(args, out):
    """per axis: the apply-free stage, apply + plain stage, the stage with a sum, plain stage + neptune_hip_dot; and a copy"""
    import torch
    from neptune_hip import _capi, apply, fields, multigrid
    lib = _capi.load()
    m = args.m
    n = m + 2
    field = lambda: fields.DeviceField((0,) * 3, (n,) * 3, _capi.F64, torch.rand((n,) * 3, dtype=torch.float64, device="cuda"))
    q, b, lo, inv, up, x = (field() for _ in range(6))
    bounds = ([1] * 3, [m + 1] * 3)
    level = multigrid.Level(None, x, bounds)
    dot = torch.zeros(1, dtype=torch.float64, device="cuda")
    launches = {"copy": lambda: q.tensor.copy_(b.tensor)}

    def apply_():
        apply.apply_builtin(_capi.BODY_LAP3D7_F64, [x], q, bounds)

    def dot_():
        _capi.check(lib.neptune_hip_dot(_capi.F64, C.byref(level.geom), b.ptr, x.ptr, dot.data_ptr(), None), "neptune_hip_dot")
    for axis in range(3):
        st = multigrid.LineStage(axis, lo, inv, up)
        launches[f"first{axis}"] = lambda st=st: multigrid.line_first(level, st, b, x)
        launches[f"apply+line{axis}"] = lambda st=st: (apply_(), multigrid.line_smooth(level, st, q, b, x))
        launches[f"linedot{axis}"] = lambda st=st: multigrid.line_smooth_dot(level, st, q, b, x, dot_out=dot)
        launches[f"line+dot{axis}"] = lambda st=st: (multigrid.line_smooth(level, st, q, b, x), dot_())
    times = {}
    for name, launch in launches.items():
        for _ in range(2):
            launch()
        x.tensor.fill_(0.5)                   # keep the values finite over the repeated updates
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.launches):
            launch()
        ev[1].record()
        torch.cuda.synchronize()
        times[name] = ev[0].elapsed_time(ev[1]) / args.launches
    out.update(field_bytes=n ** 3 * 8, launches=args.launches, ms=times)


def one(args):
    ex = _example()
    import torch
    from neptune_hip import _capi, fields, multigrid
    lib = _capi.load()
    lib.neptune_hip_init(0)
    out = {"kind": args.kind, "m": args.m}
    if args.kind == "stage":
        stage(args, out)
        print(json.dumps(out))
        return
    F = fields.DeviceField
    lines = args.kind != "cg_point"
    h = ex.hierarchy(args.m, lines)[0]
    b = F.from_numpy(ex.right_hand_side(args.m))
    x = F.empty_like(b)
    work = [F.empty_like(b) for _ in range(3)]
    x.tensor.zero_()
    _, rr0, _ = multigrid.cg_solve(h, x, b, max_iters=0, work=work, lines=lines)
    tol2 = RTOL2 * rr0
    if args.kind == "solve_lines":
        run = lambda: multigrid.solve(h, x, b, pre=2, post=2, coarse_sweeps=ex.COARSE_SWEEPS, max_cycles=ex.MAX_CYCLES, tol2=tol2)[:3]
    else:
        sweeps = 1 if args.kind == "cg_lines11" else 2
        run = lambda: multigrid.cg_solve(h, x, b, sweeps=sweeps, coarse_sweeps=ex.COARSE_SWEEPS, max_iters=ex.MAX_ITERS, tol2=tol2, work=work,
                                         lines=lines)

    def timed():
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    timed()
    res, seconds = timed()
    out.update(levels=len(h), steps=int(res[0]), ms=seconds * 1e3, rr0=rr0, rr_last=res[2], reached=bool(res[2] <= tol2))
    print(json.dumps(out))


def drive(args):
    ints = lambda s: [int(v) for v in s.split(",") if v]
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

    say(f"# tools/mgcglines_bench.py --stage-sizes {args.stage_sizes} --sizes {args.sizes} --nostage {args.nostage} --reps {args.reps}"
        + (" --parent-tree <a checkout of the parent commit>" if args.parent_tree else ""))
    for rep in range(args.reps):
        for m in ints(args.stage_sizes):
            if child("stage", m, [me, "--one", "--kind", "stage", "--m", str(m)]) is None:
                return stop()
        for m in ints(args.sizes):
            for k in SOLVE_KINDS:
                if child(k, m, [me, "--one", "--kind", k, "--m", str(m)]) is None:
                    return stop()
        if args.parent_tree and args.nostage:
            for label, tree in (("this build", REPO), ("parent build", Path(args.parent_tree).resolve())):
                cmd = [str(tree / "tools" / "mgcg_bench.py"), "--one", "--kind", "iteration", "--m", str(args.nostage), "--iters", "10"]
                if child(label, args.nostage, cmd) is None:
                    return stop()

    med = lambda m, label, key: statistics.median(key(r) for r in results[(m, label)])
    spread = lambda m, label, key: max(key(r) for r in results[(m, label)]) - min(key(r) for r in results[(m, label)])
    for m in ints(args.stage_sizes):
        rs = results[(m, "stage")]
        fb = rs[0]["field_bytes"]
        t = {k: med(m, "stage", lambda r, k=k: r["ms"][k]) for k in rs[0]["ms"]}
        sp = {k: spread(m, "stage", lambda r, k=k: r["ms"][k]) for k in rs[0]["ms"]}
        rate = 2 * fb / (t["copy"] * 1e-3)           # bytes per second of the copy: one field read, one written
        at = lambda passes: passes * fb / rate * 1e3
        say(f"{m}^3 f64 ({fb} bytes per field), median of {len(rs)} processes x {rs[0]['launches']} launches; copy {t['copy']:.3f} ms "
            f"= {rate / 1e12:.2f} TB/s:")
        for axis in range(3):
            f, al, ld, l_d = (t[f"{k}{axis}"] for k in ("first", "apply+line", "linedot", "line+dot"))
            say(f"  dim {axis}: apply-free stage {f:.3f} ms (spread {sp[f'first{axis}']:.3f}; 7 passes at the copy's rate: {at(7):.3f}) against "
                f"apply + plain stage {al:.3f} (spread {sp[f'apply+line{axis}']:.3f}; 10 passes: {at(10):.3f}): {f / al:.2f} (model 0.70); "
                f"stage with a sum {ld:.3f} (spread {sp[f'linedot{axis}']:.3f}; 9 passes: {at(9):.3f}) against plain stage + dot {l_d:.3f} "
                f"(spread {sp[f'line+dot{axis}']:.3f}; 10 passes: {at(10):.3f}): {ld / l_d:.2f} (model 0.90)")
    names = {"cg_lines11": "multigrid.cg_solve(lines=True) V(1,1), line stages", "cg_lines22": "multigrid.cg_solve(lines=True) V(2,2), line stages",
             "solve_lines": "multigrid.solve V(2,2), line stages", "cg_point": "multigrid.cg_solve V(2,2), point Jacobi"}
    for m in ints(args.sizes):
        say(f"{m}^2 f64, the operator of examples/poisson_varying_anisotropy_mgcg.py, 8 coarse sweeps, omega = 0.8, to "
            f"r.r <= {RTOL2:g} r0.r0 ({results[(m, SOLVE_KINDS[0])][0]['levels']} levels):")
        for k in SOLVE_KINDS:
            rs = results[(m, k)]
            unit = "cycles" if k.startswith("solve") else "iterations"
            ok = all(r["reached"] for r in rs)
            say(f"  {names[k]:>52}: {rs[0]['steps']} {unit}, {med(m, k, lambda r: r['ms']):.1f} ms (spread {spread(m, k, lambda r: r['ms']):.1f}), "
                + ("reached" if ok else f"NOT reached: r.r / r0.r0 = {rs[0]['rr_last'] / rs[0]['rr0']:.1e}"))
    if args.parent_tree and args.nostage:
        m = args.nostage
        key = lambda r: r["ms_per_step"]
        a, p = med(m, "this build", key), med(m, "parent build", key)
        sa, sp_ = spread(m, "this build", key), spread(m, "parent build", key)
        inside = abs(a - p) <= sp_
        say(f"multigrid.cg_solve without stages, {m}^3 f64 (tools/mgcg_bench.py iteration), ms per iteration: this build "
            f"{a:.3f} (spread {sa:.3f}), the parent's build {p:.3f} (spread {sp_:.3f}): ratio {a / p:.3f}, "
            f"{'inside' if inside else 'OUTSIDE'} the parent's own spread")
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
    ap.add_argument("--kind", choices=SOLVE_KINDS + ["stage"], default="cg_lines11")
    ap.add_argument("--m", type=int, default=1023)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--stage-sizes", default="255,511")
    ap.add_argument("--sizes", default="1023,2047")
    ap.add_argument("--nostage", type=int, default=255)
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
