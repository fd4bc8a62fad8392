#!/usr/bin/env python3
"""Leapfrog step loop: ms per step of
  (a) a host loop of the apply's ordinary __geom launches with the rotation done by the caller (what a driver could do before
      neptune_hip_step_loop_leapfrog existed: the baseline),
  (b) neptune_hip_step_loop_leapfrog restricted to single launches (three fields),
  (c) the same loop with pair launches forced on (four fields, NEPTUNE_HIP_TUNE=0: no measurement, the largest grouping),
and (auto) what the loop's own measured 3 % rule picks with four fields.
Per case, after a 1 s clock ramp, HIP events on the launch stream, best of REPS batches.  The modules are the wave equation
of examples/wave_leapfrog.py.

usage: tools/leapfrog_bench.py [--cases 512,1024,512c,1024c,8192x2] [--steps 60] [--reps 3]     one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "neptune-pde-solver_amd"))
sys.path.insert(0, str(REPO / "examples"))

CASES = {"512": ((512,) * 3, False), "1024": ((1024,) * 3, False), "512c": ((512,) * 3, True), "1024c": ((1024,) * 3, True),
         "8192x2": ((8192, 8192), False), "256": ((256,) * 3, False), "2048x2": ((2048, 2048), False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="512,1024,512c,1024c,8192x2")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import wave_leapfrog
    from neptune_hip import _capi, apply, fields
    lib = _capi.load()
    lib.neptune_hip_init(0)
    stream = torch.cuda.Stream()
    st = int(stream.cuda_stream)
    for name in args.cases.split(","):
        shape, coef = CASES[name]
        rank = len(shape)
        mod = wave_leapfrog.build(shape, 0.1, coef)
        entry = mod.geom_entry("step")
        with torch.cuda.stream(stream):
            fs = [fields.DeviceField.hashed(shape, _capi.F64, seed=s) for s in (1, 2)]
            fs += [fields.DeviceField.empty_like(fs[0]) for _ in range(2)]
            ex = [fields.DeviceField.hashed(shape, _capi.F64, seed=3)] if coef else []
            for f in fs[:2]:
                f.tensor.mul_(1e-3)               # keeps thousands of steps finite
            for f in ex:
                f.tensor.mul_(0.25).add_(0.5)
        geom = apply.geom_for(fs[:2] + ex, fs[2], ([1] * rank, [n - 1 for n in shape]))
        torch.cuda.synchronize()
        e0, e1 = lib.neptune_hip_event_create(), lib.neptune_hip_event_create()

        def timed(run):
            """best of `reps` batches of `steps` steps, ms per step"""
            best = None
            for _ in range(args.reps):
                lib.neptune_hip_event_record(e0, st)
                run()
                lib.neptune_hip_event_record(e1, st)
                lib.neptune_hip_event_sync(e1)
                ms = lib.neptune_hip_event_elapsed_ms(e0, e1) / args.steps
                best = ms if best is None else min(best, ms)
            return best

        def host_loop():
            order = [0, 1, 2]
            for _ in range(args.steps):
                cur, prev, nxt = order
                ins = (C.c_void_p * (2 + len(ex)))(fs[cur].ptr, fs[prev].ptr, *[f.ptr for f in ex])
                rc = entry.fn(C.byref(geom), ins, fs[nxt].ptr, st, None)
                assert rc == 0, rc
                order = [nxt, cur, prev]

        counts = {}

        def loop(nfields, what):
            def run():
                apply.step_loop_leapfrog(entry, geom, fs[:nfields], ex, steps=args.steps, stream=st)
                counts[what] = apply.leapfrog_launch_counts()
            return run

        # clock ramp: one second of the baseline, which also lets the single launch settle its own tile choice
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:
            host_loop()
            torch.cuda.synchronize()
        res = {"case": name, "shape": list(shape), "coef": coef, "steps": args.steps, "pair_entry": entry.info["leapfrog_symbol"]}
        res["a_host_loop_ms"] = timed(host_loop)
        loop(3, "b")()                              # warm: captures the graph
        res["b_loop_singles_ms"] = timed(loop(3, "b"))
        os.environ["NEPTUNE_HIP_TUNE"] = "0"
        loop(4, "c")()
        res["c_loop_pairs_ms"] = timed(loop(4, "c"))
        del os.environ["NEPTUNE_HIP_TUNE"]
        loop(4, "auto")()                           # measures singles against pairs once, keeps pairs if they win by 3 %
        res["auto_ms"] = timed(loop(4, "auto"))
        res["launches_singles_pairs"] = {k: list(v) for k, v in counts.items()}
        res["auto_choice"] = "pairs" if counts["auto"][1] else "singles"
        res["pairs_speedup_over_singles"] = res["b_loop_singles_ms"] / res["c_loop_pairs_ms"]
        res["rule_expects"] = "pairs" if res["c_loop_pairs_ms"] < 0.97 * res["b_loop_singles_ms"] else "singles"
        for k, v in list(res.items()):
            if isinstance(v, float):
                res[k] = round(v, 4)
        print(json.dumps(res), flush=True)
        lib.neptune_hip_event_destroy(e0)
        lib.neptune_hip_event_destroy(e1)
        del fs, ex
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
