#!/usr/bin/env python3
"""What a multigrid V-cycle costs and what it buys: the Poisson problem of examples/poisson_multigrid.py, f64,
V(2,2) with 8 coarse sweeps, against the copy ceiling and against cg_solve on the same operator, all alternated in one job.

  tools/mg_bench.py [--sizes 255,511] [--reps 3] [--cycles 10] [--limit SECONDS] [--out profiles/mg_solve.txt]
  tools/mg_bench.py --prefetch [--sizes ...]      compile every level's module into the module cache (needs no GPU)

The driver touches no GPU.  Every measurement is a fresh child process under its own `timeout -k 10 SECONDS`; the driver
checks every exit status and starts nothing more after a child that failed, was killed or ran into its limit.  Order per
size: repetition by repetition, every kind of measurement once -- so drift hits all alike.

  --one --kind KIND --m M      one measurement (what a child runs); prints one JSON line.  KIND:
      copy         neptune_hip_time_copy over one finest field: the ceiling, GB/s
      cycle        --cycles V-cycles with no tolerance, one warm-up run of the same length, wall clock around the second,
                   synchronised before and after; --graph 0 sets NEPTUNE_HIP_MG_GRAPH=0; --cut: the hierarchy cut after
                   level 2 with no sweeps there, so that levels 0 and 1 do all their work and levels >= 2 none
      solve        cycles and wall time to r . r <= 1e-16 r0 . r0
      cg           the same with apply.cg_solve (check_every 10)

Reported per size: time per cycle against passes x field bytes / copy ceiling, with the ratio (reported, not judged: no
earlier number exists); the share of a cycle spent on levels >= 2 (1 - cut / full) with and without the graph path; cycles
and time to the tolerance against cg_solve, margin: the spread (max - min) of cg_solve's own repetitions."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
RTOL2 = 1e-16
KINDS = [("copy", []), ("cycle graph", ["--graph", "1"]), ("cycle graph cut", ["--graph", "1", "--cut"]),
         ("cycle plain", ["--graph", "0"]), ("cycle plain cut", ["--graph", "0", "--cut"]), ("solve", []), ("cg", [])]


def _example():
    sys.path[:0] = [str(REPO / "neptune-pde-solver_amd"), str(REPO / "examples")]
    import poisson_multigrid as ex
    return ex


def prefetch(sizes):
    """every level's module of every size into the module cache, side by side; nothing is loaded, no GPU is touched"""
    from concurrent.futures import ThreadPoolExecutor
    ex = _example()
    from neptune_hip import lowering
    jobs = []
    for m in sizes:
        for l, ml in enumerate(ex.level_extents(m)):
            jobs.append((ex.build_text(ml)[0], l == 0))
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(lambda j: lowering.compile_module(j[0], load=False, dot_entries=j[1]), jobs))
    print(f"{len(jobs)} modules in {lowering.cache_dir()}")


def one(args):
    if args.kind.startswith("cycle"):
        os.environ["NEPTUNE_HIP_MG_GRAPH"] = str(args.graph)
    ex = _example()
    import torch
    from neptune_hip import _capi, apply, fields, lowering, multigrid
    lib = _capi.load()
    lib.neptune_hip_init(0)
    m = args.m
    n = m + 2
    f64 = torch.float64
    field = lambda t: fields.DeviceField((0,) * 3, tuple(t.shape), _capi.F64, t)
    out = {"kind": args.kind, "m": m, "label": args.label}
    if args.kind == "copy":
        a, b = torch.zeros((n,) * 3, dtype=f64, device="cuda"), torch.zeros((n,) * 3, dtype=f64, device="cuda")
        nbytes = a.numel() * 8 // 4096 * 4096          # the copy kernels move whole 16-byte vectors
        ms = min(lib.neptune_hip_time_copy(b.data_ptr(), a.data_ptr(), nbytes, fields.current_stream_ptr(), mode, 3, 20)
                 for mode in range(lib.neptune_hip_copy_mode_count()))
        if not ms > 0.0:
            raise SystemExit(f"neptune_hip_time_copy answered {ms}")
        out.update(copy_ms=ms, copy_GBps=2.0 * nbytes / ms / 1e6, copied_bytes=nbytes)
        print(json.dumps(out))
        return
    extents = ex.level_extents(m)
    if args.cut:
        extents = extents[:3]
    levels, entry0, interior0 = [], None, None
    for l, ml in enumerate(extents):
        text, interior = ex.build_text(ml)
        mod = lowering.compile_module(text, dot_entries=(l == 0))
        entry = mod.dot_entry("entry") if l == 0 else mod.geom_entry("entry")
        like = field(torch.zeros((ml + 2,) * 3, dtype=f64, device="cuda"))
        minv = torch.zeros((ml + 2,) * 3, dtype=f64, device="cuda")
        minv[1:-1, 1:-1, 1:-1] = ex.OMEGA / 6.0          # the constant diagonal: what multigrid.jacobi_weights finds by probing
        levels.append(multigrid.Level(entry, like, interior, minv=field(minv), rscale=4.0))
        if l == 0:
            entry0, interior0 = entry, interior
    h = multigrid.Hierarchy(levels)
    gen = torch.Generator(device="cuda").manual_seed(11)
    b = torch.zeros((n,) * 3, dtype=f64, device="cuda")
    b[1:-1, 1:-1, 1:-1] = torch.rand((m,) * 3, dtype=f64, device="cuda", generator=gen) - 0.5
    bf, x = field(b), field(torch.zeros_like(b))
    coarse = 0 if args.cut else ex.COARSE_SWEEPS
    out.update(levels=len(h), passes_per_cycle=ex.passes_per_cycle(len(h)), field_bytes=b.numel() * 8)

    def timed(fn):
        x.tensor.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    if args.kind.startswith("cycle"):
        K = args.cycles
        run = lambda: multigrid.solve(h, x, bf, pre=ex.PRE, post=ex.POST, coarse_sweeps=coarse, max_cycles=K, tol2=0.0, check_every=K)
        timed(run)
        res, seconds = timed(run)
        out.update(cycles=int(res[0]), counts=list(multigrid.counts()), ms_per_cycle=seconds * 1e3 / K, rr0=res[1], rr_last=res[2])
    else:
        _, rr0, _, _ = multigrid.solve(h, x, bf, max_cycles=0)
        if args.kind == "solve":
            run = lambda: multigrid.solve(h, x, bf, pre=ex.PRE, post=ex.POST, coarse_sweeps=coarse, max_cycles=ex.MAX_CYCLES,
                                          tol2=RTOL2 * rr0)
        else:
            work = [fields.DeviceField.empty_like(x) for _ in range(3)]
            run = lambda: apply.cg_solve(entry0, x, bf, interior0, ex.MAX_ITERS, RTOL2 * rr0, check_every=ex.CHECK_EVERY_CG, work=work)
        timed(run)
        res, seconds = timed(run)
        out.update(steps=int(res[0]), ms=seconds * 1e3, rr0=rr0, rr_last=res[2], reached=bool(res[2] <= RTOL2 * rr0))
    print(json.dumps(out))


def drive(args):
    sizes = [int(s) for s in args.sizes.split(",")]
    lines, results = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"# tools/mg_bench.py --sizes {args.sizes} --reps {args.reps} --cycles {args.cycles}: Poisson, f64, V(2,2), 8 coarse sweeps")
    for m in sizes:
        for rep in range(args.reps):
            for label, extra in KINDS:
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--one", "--kind",
                       label.split()[0], "--m", str(m), "--cycles", str(args.cycles), "--label", label] + extra
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    say(f"{label} m={m} repetition {rep}: exit status {p.returncode}; nothing more is started")
                    _write(args, lines)
                    return p.returncode
                out = json.loads(p.stdout.strip().splitlines()[-1])
                say(json.dumps(out))
                results.setdefault((m, label), []).append(out)
    for m in sizes:
        med = lambda label, key: statistics.median(r[key] for r in results[(m, label)])
        spread = lambda label, key: max(r[key] for r in results[(m, label)]) - min(r[key] for r in results[(m, label)])
        full = results[(m, "cycle graph")][0]
        gbps = med("copy", "copy_GBps")
        say(f"{m}^3 f64, {full['levels']} levels, {full['passes_per_cycle']:.1f} passes per cycle; copy ceiling {gbps:.0f} GB/s "
            f"(read + write), i.e. {full['field_bytes'] / (gbps * 1e6):.4f} ms per field pass")
        floor_ms = full["passes_per_cycle"] * full["field_bytes"] / (gbps * 1e6)
        for mode in ("graph", "plain"):
            t, tc = med(f"cycle {mode}", "ms_per_cycle"), med(f"cycle {mode} cut", "ms_per_cycle")
            say(f"  {mode:>5} launches: {t:.3f} ms per cycle (spread {spread(f'cycle {mode}', 'ms_per_cycle'):.3f}) against passes x "
                f"field bytes / ceiling = {floor_ms:.3f} ms: ratio {t / floor_ms:.2f}; cut after level 2: {tc:.3f} ms, share of "
                f"levels >= 2: {1.0 - tc / t:.3f}")
        cg_ms, cg_spread = med("cg", "ms"), spread("cg", "ms")
        mg_ms = med("solve", "ms")
        say(f"  to r.r <= {RTOL2:g} r0.r0: multigrid {results[(m, 'solve')][0]['steps']} cycles in {mg_ms:.1f} ms (spread "
            f"{spread('solve', 'ms'):.1f}); cg_solve {results[(m, 'cg')][0]['steps']} iterations in {cg_ms:.1f} ms (spread {cg_spread:.1f}): "
            f"{'multigrid faster beyond the margin' if mg_ms + cg_spread < cg_ms else 'NOT faster beyond the margin'} "
            f"(cg / mg = {cg_ms / mg_ms:.2f}); reached: {all(r['reached'] for r in results[(m, 'solve')] + results[(m, 'cg')])}")
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
    ap.add_argument("--kind", choices=["copy", "cycle", "solve", "cg"], default="cycle")
    ap.add_argument("--m", type=int, default=255)
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--cut", action="store_true")
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--sizes", default="255,511")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.prefetch:
        prefetch([int(s) for s in args.sizes.split(",")])
        return 0
    if args.one:
        one(args)
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
