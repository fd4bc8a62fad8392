#!/usr/bin/env python3
"""Time a time loop of a system fixture (tests/mlir_tests/systems: the 2-D shallow-water step, three unknowns; the 3-D
pair, two) on device-resident f64 fields: `--mode loop` runs neptune_hip_step_loop_system on the group's geometry-level
entry (hipGraph replay, asynchronous), `--mode host` the host loop of one lowered @entry call per step on swapped
buffers (synchronous per call unless NEPTUNE_HIP_ASYNC=1).  The run is warmed up (tile choice, graph capture), timed
from the first call to the end of a device synchronise, and reported per step.  One JSON line.  Run it in a fresh
process per measurement; --root points it at another checkout of this repository -- a build of the commit before the
system loop existed has only `--mode host`."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["swe", "pair"])
    ap.add_argument("n", type=int, help="cells per dimension")
    ap.add_argument("--mode", choices=["loop", "host"], default="loop")
    ap.add_argument("--root", default=str(HERE), help="checkout whose package and libraries run the module")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    root = Path(a.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(HERE / "tests"), str(root / "tools"), str(root)]
    import numpy as np
    import torch
    import group_cases as gc
    import system_loop_cases as sc
    from neptune_hip import _capi, apply, fields, lowering
    shape = (a.n,) * (2 if a.kind == "swe" else 3)
    mod = lowering.compile_module(gc.variant(a.kind, shape))
    if a.kind == "swe":
        cur = [torch.from_numpy(x).cuda() for x in sc.loop_inputs(a.kind, shape, np.float64)]
    else:   # the hash fields of sc.loop_inputs, filled on the device
        cur = [fields.DeviceField.hashed(shape, _capi.F64, seed=11 + k).tensor for k in range(2)]
    nxt = [t.clone() for t in cur]
    bounds = ([1] * len(shape), [n - 1 for n in shape])

    def run(steps):
        nonlocal cur, nxt
        if a.mode == "loop":
            newest = apply.step_loop_system(entry, bounds, cur, nxt, steps=steps)
            if newest[0] is nxt[0]:
                cur, nxt = nxt, cur
        else:
            for _ in range(steps):
                mod.call("entry", *nxt, *cur)
                cur, nxt = nxt, cur
        torch.cuda.synchronize()

    entry = mod.group_entry("entry") if a.mode == "loop" else None
    run(a.warmup - a.warmup % 2)          # an even count: the timed run starts on the buffers the warm-up started on
    t0 = time.perf_counter()
    run(a.steps)
    per = (time.perf_counter() - t0) / a.steps
    out = {"kind": a.kind, "n": a.n, "mode": a.mode, "label": a.label, "root": str(root),
           "async": os.environ.get("NEPTUNE_HIP_ASYNC", ""), "steps": a.steps, "us_per_step": round(per * 1e6, 3),
           "tb_s_over_2m_fields": round(2 * len(cur) * int(np.prod(shape)) * 8 / per / 1e12, 3),
           "finite": all(bool(torch.isfinite(t).all()) for t in cur)}
    if a.mode == "loop":
        out["loop_counts"] = list(apply.system_loop_counts())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
