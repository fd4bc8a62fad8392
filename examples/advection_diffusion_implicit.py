#!/usr/bin/env python3
"""Backward-Euler steps of advection-diffusion in 3-D with first-order upwinding:

    u' - u + dt * (a . grad_upwind(u') - D lap(u')) = 0       on the interior, u' = 0 on the rim

With kappa = dt D / h^2 = 1 and c = dt a / h = (4, 2, 1) one step is the linear system

    (1 + 6 kappa + c0 + c1 + c2) u' - sum_d (kappa + c_d) u'<p - e_d> - sum_d kappa u'<p + e_d> = u

whose matrix is not symmetric: the upwinded advection weights the lower neighbours 5, 3 and 2 and the upper ones 1.  Conjugate
gradients need a symmetric positive definite operator and quietly diverge here; BiCGStab does not.
neptune_hip.apply.bicgstab_solve (neptune_hip_bicgstab_solve) keeps the vectors and the scalars of the iteration
on the device: 21 field passes per iteration, one read-back per `check_every` iterations.

The same driver -- same recurrences, same blocks of `check_every` iterations, same test on r . r -- runs on the CPU oracle
for a small grid and must take the same number of iterations in every step and agree to rounding; what cg_solve does on the
first step's system is printed beside it.  Then iterations and time per step are printed for the size asked for.

usage: examples/advection_diffusion_implicit.py [N]        (default 256^3)"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "oracle"))

RTOL2 = 1e-16      # stop when r . r <= RTOL2 * (r . r of the first guess)
CHECK_EVERY = 4
MAX_ITERS = 200
STEPS = 3
KAPPA = 1.0
C_ADV = (4.0, 2.0, 1.0)


def build_text(n):
    """@entry(out, u): out = the backward-Euler operator above on the interior, copy-through on the rim"""
    import neptune as nep
    nep.reset()
    box = ([0, 0, 0], [n, n, n])
    interior = ([1, 1, 1], [n - 1, n - 1, n - 1])
    c = nep.get_compiler()
    c.start_function("entry", [("memref", 3), ("memref", 3)])
    fout = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    u = nep.load(nep.wrap(nep.Expr(c.get_function_arg(1)), box))
    centre = 1.0 + 6.0 * KAPPA + sum(C_ADV)
    lo = [KAPPA + cd for cd in C_ADV]

    @nep.apply(inputs=[u], bounds=interior)
    def backward_euler(x):
        return x[0, 0, 0] * centre - (x[-1, 0, 0] * lo[0] + x[0, -1, 0] * lo[1] + x[0, 0, -1] * lo[2]
                                      + x[1, 0, 0] + x[0, 1, 0] + x[0, 0, 1])

    nep.store(backward_euler, fout)
    c.create_return(nep.unwrap(fout)._handle)
    c.end_function()
    text = c.dump()
    nep.reset()
    return text, interior


def initial_state(n):
    """a smooth bump that vanishes on the rim"""
    x = (np.arange(n) + 0.5) / n
    s = np.sin(np.pi * x) ** 2
    u = s[:, None, None] * s[None, :, None] * s[None, None, :]
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    return u


def bicgstab_on_oracle(A, x, b, sl):
    """the driver on the CPU oracle: BiCGStab as neptune_hip_bicgstab_solve defines it -> (iterations, solution)"""
    r = np.zeros_like(b)
    r[sl] = b[sl] - A(x)[sl]
    rh, p = r.copy(), r.copy()
    rho = rr = float(np.sum(r * r))
    tol2, done = RTOL2 * rr, 0
    while done < MAX_ITERS and rr > tol2:
        for _ in range(min(CHECK_EVERY, MAX_ITERS - done)):
            v = A(p)
            rv = float(np.sum(rh * v))
            alpha = 0.0 if (rho == 0.0 or rv == 0.0) else rho / rv
            s = r - alpha * v
            t = A(s)
            ts, tt = float(np.sum(t[sl] * s[sl])), float(np.sum(t * t))
            omega = 0.0 if tt == 0.0 else ts / tt
            x = (x + alpha * p) + omega * s
            r = s - omega * t
            rho_new, rr = float(np.sum(rh * r)), float(np.sum(r * r))
            beta = 0.0 if (rho == 0.0 or rv == 0.0 or omega == 0.0) else (rho_new / rho) * (alpha / omega)
            p = r + beta * (p - omega * v)
            rho = rho_new
            done += 1
    return done, x


def steps_on_oracle(text, u0, interior):
    import neptune_oracle as oracle
    m = oracle.Module.parse(text)
    sl = tuple(slice(lo, hi) for lo, hi in zip(*interior))

    def A(v):
        out = np.zeros_like(v)
        m.call("entry", out, v)
        return out

    u, iters = u0.copy(), []
    for _ in range(STEPS):
        it, u = bicgstab_on_oracle(A, u.copy(), u, sl)      # the old state is the right-hand side and the first guess
        iters.append(it)
    return iters, u


def steps_on_gpu(entry, u0, interior):
    """-> (iterations per step, the last state as numpy, seconds in bicgstab_solve, (fused, fallback) iterations of the last step)"""
    import torch
    from neptune_hip import apply, fields
    F = fields.DeviceField
    x, b = F.from_numpy(u0), F.from_numpy(u0)
    work = [F.empty_like(x) for _ in range(5)]
    iters, seconds = [], 0.0
    for _ in range(STEPS):
        b.tensor.copy_(x.tensor)
        _, rr0, _ = apply.bicgstab_solve(entry, x, b, interior, 0, 0.0, work=work)      # r . r of the first guess
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done, _, _ = apply.bicgstab_solve(entry, x, b, interior, MAX_ITERS, RTOL2 * rr0, check_every=CHECK_EVERY, work=work)
        seconds += time.perf_counter() - t0
        iters.append(done)
    return iters, x.numpy(), seconds, apply.cg_counts()[:2]


def cg_on_the_same_system(entry, u0, interior, iters=40):
    """what cg_solve does on the first step's system: -> (rr0, r . r of its recurrence after `iters` iterations, the true
    |b - A(x)|^2 then)"""
    import torch
    from neptune_hip import apply, fields
    F = fields.DeviceField
    x, b, out = F.from_numpy(u0), F.from_numpy(u0), F.from_numpy(u0)
    _, rr0, rr_last = apply.cg_solve(entry, x, b, interior, iters, 0.0, check_every=iters)
    apply.apply_builtin(entry, [x], out, interior)
    torch.cuda.synchronize()
    sl = tuple(slice(lo, hi) for lo, hi in zip(*interior))
    true = float(np.sum((u0[sl] - out.numpy()[sl]) ** 2))
    return rr0, rr_last, true


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    from neptune_hip import lowering

    # 1. a grid the CPU oracle solves in seconds: same iteration counts, same solution to rounding
    ns = 40
    text, interior = build_text(ns)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    u0 = initial_state(ns)
    iters, got, _, counts = steps_on_gpu(entry, u0, interior)
    want_iters, want = steps_on_oracle(text, u0, interior)
    err = float(np.max(np.abs(got - want)))
    ok = iters == want_iters and err <= 1e-12
    print(f"{ns}^3 BiCGStab, {STEPS} backward-Euler steps: {iters} iterations (oracle {want_iters}), max |u - oracle| = {err:.2e}, "
          f"iterations fused / fallback in the last step: {counts}")
    rr0, rr_cg, true_cg = cg_on_the_same_system(entry, u0, interior)
    print(f"{ns}^3 cg_solve on the first step's system, 40 iterations: recurrence r.r / r0.r0 = {rr_cg / rr0:.2e}, "
          f"true |b - A x|^2 / r0.r0 = {true_cg / rr0:.2e} (not a solve: the operator is not symmetric)")
    # 2. the size asked for
    text, interior = build_text(n)
    entry = lowering.compile_module(text, dot_entries=True).dot_entry("entry")
    u0 = initial_state(n)
    steps_on_gpu(entry, u0, interior)                                      # warm: graphs, workspaces
    iters, _, seconds, counts = steps_on_gpu(entry, u0, interior)
    total = max(sum(iters), 1)
    print(f"{n}^3 BiCGStab, {STEPS} backward-Euler steps: {iters} iterations to r.r <= {RTOL2:g} r0.r0 in {seconds * 1e3:.1f} ms "
          f"({seconds / total * 1e3:.3f} ms per iteration), iterations fused / fallback in the last step: {counts}")
    print("agrees with the oracle:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
