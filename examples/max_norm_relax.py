#!/usr/bin/env python3
"""The damped-Jacobi relaxation of jacobi_relax.py, stopped in the max norm:

    u <- A(u) = (1 - w) u + w/4 (u_n + u_s + u_w + u_e + h^2 f)        until  R = max |A(u) - u| <= tol

R is `neptune.reduce_max` of a single-use apply, so the lowering fuses the two: one read-only launch per check, the
residual field never exists in memory.  The l2 update norm of jacobi_relax.py hides a single cell that does
not converge; the max norm does not.  The module is built with the Python DSL -- `abs()` in the kernel body is
math.absf, and reduce_max puts the lowering option line reduce-kinds into the module text, so it compiles unasked.

max folds exactly in any order, so a NumPy restatement of the same loop (same operations in the same order) must see
the same R bit for bit and stop at the same step: that is checked on a small grid; then the step count and the cost
of a check are printed for the size asked for.

usage: examples/max_norm_relax.py [N] [MAX_STEPS] [TOL]        (default 1024 x 1024, 4000 steps, tol = 1e-7)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))

OMEGA = 0.8


def build_text(n):
    """@entry(out, u, f): one sweep over the interior (f carries h^2); @resid(u, f) -> max |A(u) - u| over the interior"""
    import neptune as nep
    nep.reset()
    box = ([0, 0], [n, n])
    interior = ([1, 1], [n - 1, n - 1])
    c = nep.get_compiler()

    def sweep_of(x, rhs):
        return x[0, 0] * (1.0 - OMEGA) + (x[-1, 0] + x[1, 0] + x[0, -1] + x[0, 1] + rhs[0, 0]) * (OMEGA / 4.0)

    c.start_function("entry", [("memref", 2), ("memref", 2), ("memref", 2)])
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u = nep.load(nep.wrap(nep.Expr(c.get_function_arg(1)), box))
    f = nep.load(nep.wrap(nep.Expr(c.get_function_arg(2)), box))

    @nep.apply(inputs=[u, f], bounds=interior)
    def sweep(x, rhs):
        return sweep_of(x, rhs)

    nep.store(sweep, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()

    c.start_function("resid", [("memref", 2), ("memref", 2)])
    u = nep.load(nep.wrap(nep.Expr(c.get_function_arg(0)), box))
    f = nep.load(nep.wrap(nep.Expr(c.get_function_arg(1)), box))

    @nep.apply(inputs=[u, f], bounds=interior)
    def defect(x, rhs):
        return abs(sweep_of(x, rhs) - x[0, 0])

    c.create_return(nep.reduce_max(defect, interior)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text


def problem(n):
    """a smooth source, zero Dirichlet rim, zero first guess"""
    x = (np.arange(n) + 0.5) / n
    h2 = 1.0 / (n * n)
    f = h2 * 2.0 * np.pi ** 2 * np.outer(np.sin(np.pi * x), np.sin(np.pi * x))
    return np.zeros((n, n)), f


def sweep_numpy(u, f):
    """A(u) on the interior, the operations of the kernel body in its order (no FMA); the rim is copied through"""
    out = u.copy()
    s = u[:-2, 1:-1] + u[2:, 1:-1]
    s = s + u[1:-1, :-2]
    s = s + u[1:-1, 2:]
    s = s + f[1:-1, 1:-1]
    out[1:-1, 1:-1] = u[1:-1, 1:-1] * (1.0 - OMEGA) + s * (OMEGA / 4.0)
    return out


def relax_numpy(u0, f, max_steps, check_every, tol, trace=None):
    """-> (steps done, last R, state): R = max |A(u) - u| over the interior, checked every check_every steps; trace: a
    list that receives R of every check"""
    cur, done, r = u0, 0, float("inf")
    while done < max_steps:
        for _ in range(min(check_every, max_steps - done)):
            cur = sweep_numpy(cur, f)
            done += 1
        r = float(np.max(np.abs(sweep_numpy(cur, f) - cur)[1:-1, 1:-1]))
        if trace is not None:
            trace.append(r)
        if r <= tol:
            break
    return done, r, cur


def relax_gpu(mod, u0, f, max_steps, check_every, tol):
    """the same loop on the device: @entry steps between two buffers, @resid is one fused read-only launch per check"""
    import torch
    a, b = torch.from_numpy(u0).cuda(), torch.from_numpy(u0).cuda()   # both carry the rim
    ff = torch.from_numpy(f).cuda()
    done, r, checks, check_s = 0, float("inf"), 0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while done < max_steps:
        for _ in range(min(check_every, max_steps - done)):
            mod.call("entry", b, a, ff)
            a, b = b, a
            done += 1
        t1 = time.perf_counter()
        r = mod.call("resid", a, ff)          # blocking: the scalar comes back to the host
        check_s += time.perf_counter() - t1
        checks += 1
        if r <= tol:
            break
    torch.cuda.synchronize()
    return done, r, a.cpu().numpy(), time.perf_counter() - t0, checks, check_s


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    max_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    tol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-7
    from neptune_hip import lowering

    # 1. a grid NumPy steps in a moment: same stop step, same R, same field, bit for bit
    ns = 96
    text = build_text(ns)
    assert text.startswith("// neptune-hip-option: reduce-kinds\n")
    mod = lowering.compile_module(text)
    fused = [a for a in mod.report["applies"] if a["function"] == "resid"]
    assert [a["kernel"] for a in fused] == ["reduce"] and fused[0]["reduce_kind"] == "max", fused
    u0, f = problem(ns)
    # a tolerance between R of steps 123 and 124: check_every 1 stops after 124 steps, check_every 8 after 128
    trace = []
    relax_numpy(u0, f, 124, 1, 0.0, trace)
    small_tol = float(np.sqrt(trace[122] * trace[123]))
    ok = True
    for ce in (1, 8):
        want_done, want_r, want_u = relax_numpy(u0, f, 400, ce, small_tol)
        done, r, got, _, _, _ = relax_gpu(mod, u0, f, 400, ce, small_tol)
        same = (done == want_done and 0 < done < 400 and np.float64(r).tobytes() == np.float64(want_r).tobytes()
                and np.array_equal(got.view(np.uint64), want_u.view(np.uint64)))
        ok = ok and same
        print(f"{ns} x {ns}, check_every {ce}: GPU stops after {done} steps (NumPy {want_done}), R = {r!r} (NumPy {want_r!r}), "
              f"R and fields bit-identical: {same}")
    # 2. the size asked for
    text = build_text(n)
    mod = lowering.compile_module(text)
    u0, f = problem(n)
    relax_gpu(mod, u0, f, 16, 8, 0.0)                 # warm
    for ce in (1, 8):
        done, r, _, seconds, checks, check_s = relax_gpu(mod, u0, f, max_steps, ce, tol)
        print(f"{n} x {n}, check_every {ce}: {done} steps, R = {r:.6e}, {seconds / max(done, 1) * 1e6:.1f} us/step, "
              f"{checks} checks at {check_s / max(checks, 1) * 1e6:.1f} us each (one fused read-only launch + the scalar's copy back)")
    print("agrees with NumPy:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
