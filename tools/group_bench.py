#!/usr/bin/env python3
"""Time one call of a system fixture's lowered @entry at production size (tests/mlir_tests/systems: the 2-D shallow-water
step, 8192^2 f64, three results; the 3-D pair, 512^3 f64, two results) on device-resident fields, ending in a device
synchronise, after a warm-up that also lets the launcher measure its tile.  One JSON line.  Run it in a fresh process per
measurement (tuned choices are cached per process); --root points it at another checkout of this repository -- a build
of the commit before groups existed runs the same module text with one launch per member -- and NEPTUNE_HIP_NO_GROUPS=1
forces that path in this build."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["swe", "pair"])
    ap.add_argument("--root", default=str(HERE), help="checkout whose package and libraries run the module")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    root = Path(a.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(HERE / "tests"), str(root / "tools"), str(root)]
    import numpy as np
    import torch
    import group_cases as gc
    from neptune_hip import _capi, lowering
    shape = {"swe": (8192, 8192), "pair": (512, 512, 512)}[a.kind]
    mod = lowering.compile_module(gc.variant(a.kind, shape))
    ins = [torch.from_numpy(x).cuda() for x in gc.inputs(a.kind, shape, np.float64)]
    outs = [torch.empty_like(x) for x in ins]
    for _ in range(a.warmup):
        mod.call("entry", *outs, *ins)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mod.call("entry", *outs, *ins)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    import ctypes as C
    last = _capi.LaunchCfg()
    _capi.load().neptune_hip_last_launch(C.byref(last))
    n, m = len(ins), len(outs)
    cells = int(np.prod(shape))
    med = statistics.median(ms)
    print(json.dumps({"kind": a.kind, "label": a.label, "root": str(root), "no_groups": os.environ.get("NEPTUNE_HIP_NO_GROUPS", ""),
                      "groups": len(mod.report.get("groups", [])), "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                      "tb_s_over_n_plus_m_fields": round((n + m) * cells * 8 / (med * 1e-3) / 1e12, 3),
                      "last_launch": [last.kernel, last.variant, last.chunk]}))


if __name__ == "__main__":
    main()
