#!/usr/bin/env python3
"""Acoustic wave equation, 8th order in space (the 25-point star of seismic modelling), leapfrog in time:

    u_next = 2 u - u_prev + (c dt / h)^2 * L8(u)

written with the Python DSL as ONE two-input apply per step: `u` is read at 25 offsets (radius 4, the march
kernel's widest 3-D footprint), `u_prev` at the centre only.  Three device fields rotate inside
neptune_hip_step_loop_leapfrog -- no per-step synchronisation, long runs replay a hipGraph; radius 4 is beyond the
two-steps-per-pass kernel (examples/wave_leapfrog.py shows that one), so every step is one launch.  Nothing else is
allocated or copied; the energy-like diagnostic sum(u^2) is a fused reduce(apply).

usage: examples/wave_25pt.py [N] [STEPS]        (default 256^3, 100 steps)"""
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))

# 8th-order central second-derivative weights for offsets 0..4
W = [-205.0 / 72.0, 8.0 / 5.0, -1.0 / 5.0, 8.0 / 315.0, -1.0 / 560.0]
R = 4


def build(n, courant2):
    import neptune as nep
    nep.reset()
    box = ([0, 0, 0], [n, n, n])
    interior = ([R] * 3, [n - R] * 3)
    c = nep.get_compiler()
    c.start_function("step", [("memref", 3), ("memref", 3), ("memref", 3)])
    f_next, f_cur, f_prev = (nep.wrap(nep.Expr(c.get_function_arg(k)), box) for k in range(3))
    u, u_prev = nep.load(f_cur), nep.load(f_prev)

    @nep.apply(inputs=[u, u_prev], bounds=interior)
    def leapfrog(x, xp):
        lap = (3.0 * W[0]) * x[0, 0, 0]
        for s in range(1, R + 1):
            ring = x[-s, 0, 0] + x[s, 0, 0] + x[0, -s, 0] + x[0, s, 0] + x[0, 0, -s] + x[0, 0, s]
            lap = lap + W[s] * ring
        return 2.0 * x[0, 0, 0] - xp[0, 0, 0] + courant2 * lap

    nep.store(leapfrog, f_next)
    c.create_return(nep.unwrap(f_next)._handle)
    c.end_function()

    c.start_function("norm2", [("memref", 3)])
    v = nep.load(nep.wrap(nep.Expr(c.get_function_arg(0)), box))

    @nep.apply(inputs=[v], bounds=box)
    def square(x):
        return x[0, 0, 0] * x[0, 0, 0]

    c.create_return(nep.reduce_sum(square)._handle)
    c.end_function()
    mod = nep.jit_compile(c)
    nep.reset()
    return mod


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    import torch
    from neptune_hip import apply, fields
    mod = build(n, 0.1)
    kernels = [(a["function"], a["kernel"]) for a in mod.report["applies"]]
    print("kernels:", kernels)
    g = torch.arange(n, dtype=torch.float64, device="cuda") - n / 2
    pulse = torch.exp(-(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) / 18.0)   # centred Gaussian
    fs = [pulse.clone(), pulse.clone(), torch.zeros_like(pulse)]                  # u(0), u(-1): starts at rest; scratch
    entry = mod.geom_entry("step")                                                # the leapfrog apply, callable with a geometry
    f0 = fields.DeviceField((0, 0, 0), (n, n, n), tensor=fs[0])
    geom = apply.geom_for([f0, f0], f0, ([R] * 3, [n - R] * 3))
    e0 = mod.call("norm2", fs[0])
    warm = [f.clone() for f in fs]                                                # settles the launch's tile choice off the clock
    apply.step_loop_leapfrog(entry, geom, warm, steps=steps)
    torch.cuda.synchronize()
    del warm
    t0 = time.perf_counter()
    cur, prev = apply.step_loop_leapfrog(entry, geom, fs, steps=steps)            # -> which fields hold u(steps), u(steps - 1)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / steps
    cur = fs[cur]
    e1 = mod.call("norm2", cur)
    rim_quiet = bool(cur[:R].abs().max() < 1e-6)           # the pulse has not reached the (fixed) rim
    finite = bool(torch.isfinite(cur).all())
    print(f"{n}^3, {steps} steps: {per * 1e3:.3f} ms/step, {(n - 2 * R) ** 3 / per / 1e9:.1f} Gcell/s, "
          f"{3 * n ** 3 * 8 / per / 1e12:.2f} TB/s (3 fields); sum u^2 {e0:.6f} -> {e1:.6f}; stable: {finite and e1 < 4 * e0}"
          f"{'' if rim_quiet else ' (pulse reached the rim)'}")


if __name__ == "__main__":
    main()
