#!/usr/bin/env python3
"""Reaction-diffusion with a rough reaction coefficient in 3-D:

    (12 + w) u - (six neighbours of u) = b      on the interior, u = 0 on the rim

where w is a coefficient FIELD (input 1 of the apply) that jumps from cell to cell between 0, 16, 256 and 4096.  The operator
is symmetric positive definite, but its diagonal spans 12 .. 4108 and plain conjugate gradients pay for that contrast in
iterations.  A diagonal (Jacobi) preconditioner removes most of it and costs almost nothing: neptune_hip.apply.cg_solve
with minv=jacobi_minv(...) forms z = minv * r in registers inside the two flat kernels that stream r anyway
(neptune_hip_pcg_solve), 13 field passes per iteration against 11.

jacobi_minv probes the lowered operator's diagonal with coloured unit vectors -- no second description of the operator is
needed.  The same driver -- same recurrences, same blocks of `check_every` iterations, same test on r . r -- runs on the CPU
oracle for a small grid and must take the same number of iterations, with and without the preconditioner, and agree to
rounding; then iterations and time to a relative r . r of 1e-16 are printed for the size asked for.

usage: examples/pcg_variable_coeff.py [N]        (default 256^3)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

RTOL2 = 1e-16      # stop when r . r <= RTOL2 * (r . r of the first guess)
CHECK_EVERY = 4
MAX_ITERS = 400
W_VALUES = np.array([0.0, 16.0, 256.0, 4096.0])


def build_text(n):
    """@entry(out, u, w): out = (12 + w) u - (six neighbours) on the interior, copy-through on the rim"""
    import neptune as nep
    nep.reset()
    box = ([0, 0, 0], [n, n, n])
    interior = ([1, 1, 1], [n - 1, n - 1, n - 1])
    c = nep.get_compiler()
    c.start_function("entry", [("memref", 3), ("memref", 3), ("memref", 3)])
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u = nep.load(nep.wrap(nep.Expr(c.get_function_arg(1)), box))
    w = nep.load(nep.wrap(nep.Expr(c.get_function_arg(2)), box))

    @nep.apply(inputs=[u, w], bounds=interior)
    def reaction_diffusion(x, k):
        return x[0, 0, 0] * (k[0, 0, 0] + 12.0) - (x[-1, 0, 0] + x[1, 0, 0] + x[0, -1, 0] + x[0, 1, 0] + x[0, 0, -1] + x[0, 0, 1])

    nep.store(reaction_diffusion, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text, interior


def problem(n):
    """-> (w, b): the coefficient drawn per cell, a smooth right-hand side; deterministic"""
    rng = np.random.default_rng(7)
    w = W_VALUES[rng.integers(0, len(W_VALUES), size=(n, n, n))]
    x = (np.arange(n) + 0.5) / n
    s = np.sin(np.pi * x)
    b = s[:, None, None] * s[None, :, None] * s[None, None, :]
    return w, b


def solve_on_oracle(text, w, b, interior, minv):
    """the driver on the CPU oracle -> (iterations, solution); minv: the preconditioner's field, or None for plain CG"""
    import neptune_oracle as oracle
    m = oracle.Module.parse(text)
    sl = tuple(slice(lo, hi) for lo, hi in zip(*interior))
    if minv is None:
        minv = np.ones_like(b)

    def A(v):
        out = np.zeros_like(v)
        m.call("entry", out, v, w)
        return out

    x = np.zeros_like(b)
    r = np.zeros_like(b)
    r[sl] = b[sl] - A(x)[sl]
    p = minv * r
    rz, rr = float(np.sum(r * p)), float(np.sum(r * r))
    tol2, done = RTOL2 * rr, 0
    while done < MAX_ITERS and rr > tol2:
        for _ in range(min(CHECK_EVERY, MAX_ITERS - done)):
            q = A(p)
            pq = float(np.sum(q[sl] * p[sl]))
            broken = rz == 0.0 or pq == 0.0
            alpha = 0.0 if broken else rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = minv * r
            rz_new, rr = float(np.sum(r * z)), float(np.sum(r * r))
            beta = 0.0 if broken else rz_new / rz
            p = z + beta * p
            rz = rz_new
            done += 1
    return done, x


def oracle_diagonal(text, w, interior):
    """the probing of apply.operator_diagonal on the oracle (reach 1: 27 colours)"""
    import itertools
    import neptune_oracle as oracle
    m = oracle.Module.parse(text)
    diag = np.zeros_like(w)
    for colour in itertools.product(range(3), repeat=3):
        cells = tuple(slice(lo + c, hi, 3) for lo, hi, c in zip(*interior, colour))
        probe, out = np.zeros_like(w), np.zeros_like(w)
        probe[cells] = 1.0
        m.call("entry", out, probe, w)
        diag[cells] = out[cells]
    return diag


def solve_on_gpu(entry, w, b, interior, precondition):
    """-> (iterations, solution as numpy, seconds in cg_solve, seconds building the preconditioner, (fused, fallback)
    iterations, the preconditioner's field or None)"""
    import torch
    from neptune_hip import apply, fields
    F = fields.DeviceField
    wf, bf = F.from_numpy(w), F.from_numpy(b)
    x = F.from_numpy(np.zeros_like(b))
    work = [F.empty_like(x) for _ in range(3)]
    minv, setup = None, 0.0
    if precondition:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        minv = apply.jacobi_minv(entry, x, interior, others=[wf])
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0
    _, rr0, _ = apply.cg_solve(entry, x, bf, interior, 0, 0.0, others=[wf], work=work, minv=minv)    # r . r of the first guess
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done, _, _ = apply.cg_solve(entry, x, bf, interior, MAX_ITERS, RTOL2 * rr0, check_every=CHECK_EVERY, others=[wf], work=work,
                                minv=minv)
    seconds = time.perf_counter() - t0
    return done, x.numpy(), seconds, setup, apply.cg_counts()[:2], minv


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    from neptune_hip import lowering

    # 1. a grid the CPU oracle solves in seconds: same iteration counts, same solution to rounding, same diagonal
    ns = 40
    text, interior = build_text(ns)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    w, b = problem(ns)
    ok = True
    for pre in (False, True):
        it, got, _, _, counts, minv = solve_on_gpu(entry, w, b, interior, pre)
        ref_minv = None
        if pre:
            diag = oracle_diagonal(text, w, interior)
            sl = tuple(slice(lo, hi) for lo, hi in zip(*interior))
            ref_minv = np.ones_like(w)
            ref_minv[sl] = 1.0 / diag[sl]
            ok = ok and np.array_equal(minv.numpy(), ref_minv) and np.array_equal(diag[sl], 12.0 + w[sl])
        want_it, want = solve_on_oracle(text, w, b, interior, ref_minv)
        err = float(np.max(np.abs(got - want)))
        ok = ok and it == want_it and err <= 1e-12
        print(f"{ns}^3 {'Jacobi-preconditioned' if pre else 'plain':>21} CG: {it} iterations (oracle {want_it}), "
              f"max |u - oracle| = {err:.2e}, iterations fused / fallback: {counts}")
    # 2. the size asked for
    text, interior = build_text(n)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    w, b = problem(n)
    for pre in (False, True):
        solve_on_gpu(entry, w, b, interior, pre)                                      # warm: graphs, workspaces
        it, _, seconds, setup, counts, _ = solve_on_gpu(entry, w, b, interior, pre)
        print(f"{n}^3 {'Jacobi-preconditioned' if pre else 'plain':>21} CG: {it} iterations to r.r <= {RTOL2:g} r0.r0 in "
              f"{seconds * 1e3:.1f} ms ({seconds / max(it, 1) * 1e3:.3f} ms per iteration"
              + (f", {setup * 1e3:.1f} ms to probe the diagonal" if pre else "") + f"), iterations fused / fallback: {counts}")
    print("agrees with the oracle:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
