#!/usr/bin/env python3
"""Second-order wave equation, 7-point Laplacian in 3-D, leapfrog in time:

    u_next = 2 u - u_prev + (c dt / h)^2 * L(u)

written with the Python DSL as ONE apply per step over (u, u_prev) -- or (u, u_prev, c2) with a variable wave speed, the
coefficient field read at the centre only -- and stepped by neptune_hip_step_loop_leapfrog: the fields rotate inside the
library, long runs replay a hipGraph, and with a fourth field the loop may take TWO steps per pass over HBM
(csrc/kernels/apply_march2.hpp, leapfrog form) where that measures faster.  Both u(steps) and u(steps - 1) come back.

usage: examples/wave_leapfrog.py [N] [STEPS] [--c2]        (default 256^3, 100 steps, constant wave speed)"""
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))


def build(shape, courant2=0.1, variable_c2=False):
    """-> LoweredModule with @step(next, cur, prev[, c2]) holding the leapfrog apply (rank 2: the 5-point Laplacian,
    rank 3: the 7-point one) and @norm2(u) = sum u^2"""
    import neptune as nep
    nep.reset()
    rank = len(shape)
    box = ([0] * rank, list(shape))
    interior = ([1] * rank, [n - 1 for n in shape])
    nargs = 4 if variable_c2 else 3
    c = nep.get_compiler()
    c.start_function("step", [("memref", rank)] * nargs)
    fields = [nep.wrap(nep.Expr(c.get_function_arg(k)), box) for k in range(nargs)]
    inputs = [nep.load(f) for f in fields[1:]]
    zero = (0,) * rank

    def offset(d, s):
        return tuple(s if k == d else 0 for k in range(rank))

    def body(x, xp, *c2):
        lap = (-2.0 * rank) * x[zero]
        for d in range(rank):
            lap = lap + (x[offset(d, -1)] + x[offset(d, 1)])
        k = courant2 * c2[0][zero] if c2 else courant2
        return 2.0 * x[zero] - xp[zero] + k * lap

    leapfrog = nep.apply(inputs=inputs, bounds=interior)(body)
    nep.store(leapfrog, fields[0])
    c.create_return(nep.unwrap(fields[0])._handle)
    c.end_function()

    c.start_function("norm2", [("memref", rank)])
    v = nep.load(nep.wrap(nep.Expr(c.get_function_arg(0)), box))

    @nep.apply(inputs=[v], bounds=box)
    def square(x):
        return x[zero] * x[zero]

    c.create_return(nep.reduce_sum(square)._handle)
    c.end_function()
    mod = nep.jit_compile(c)
    nep.reset()
    return mod


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 256
    steps = int(args[1]) if len(args) > 1 else 100
    variable = "--c2" in sys.argv
    import torch
    from neptune_hip import apply, fields
    shape = (n, n, n)
    mod = build(shape, 0.1, variable)
    entry = mod.geom_entry("step")
    print("pair entry:", entry.info["leapfrog_symbol"] or "none")
    g = torch.arange(n, dtype=torch.float64, device="cuda") - n / 2
    pulse = torch.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / 18.0)   # centred Gaussian
    fs = [pulse.clone(), pulse.clone(), torch.zeros_like(pulse), torch.zeros_like(pulse)]                # starts at rest
    extra = [1.0 + 0.5 * torch.tanh(g / (n / 8))[:, None, None].expand(n, n, n).contiguous()] if variable else []
    f0 = fields.DeviceField((0, 0, 0), shape, tensor=fs[0])
    geom = apply.geom_for([f0] * (2 + len(extra)), f0, ([1, 1, 1], [n - 1] * 3))
    e0 = mod.call("norm2", fs[0])
    cur, prev = apply.step_loop_leapfrog(entry, geom, fs, extra, steps=steps)       # warm: measures the grouping, captures the graph
    torch.cuda.synchronize()
    fs = [fs[cur], fs[prev]] + [f for k, f in enumerate(fs) if k not in (cur, prev)]
    t0 = time.perf_counter()
    cur, prev = apply.step_loop_leapfrog(entry, geom, fs, extra, steps=steps)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / steps
    singles, pairs = apply.leapfrog_launch_counts()
    e1 = mod.call("norm2", fs[cur])
    finite = bool(torch.isfinite(fs[cur]).all()) and bool(torch.isfinite(fs[prev]).all())
    print(f"{n}^3, {2 * steps} steps: {pairs} pair + {singles} single launches in the timed run "
          f"({'two steps per pass' if pairs else 'one launch per step'}), {per * 1e3:.3f} ms/step, "
          f"{(n - 2) ** 3 / per / 1e9:.1f} Gcell/s; sum u^2 {e0:.6f} -> {e1:.6f}; stable: {finite and e1 < 4 * e0}")


if __name__ == "__main__":
    main()
