#!/usr/bin/env python3
"""Record the device scalars of the solves listed in tests/solver_trace_cases.py as exact bits (float.hex()) into
tests/golden/solver_traces.json, the fixture of tests/test_solver_traces_gpu.py.  Needs a GPU.  Run it with the library whose
sums are to be pinned -- before a change of the solvers' kernels, not after: the test then holds the change to those bits.

  --root DIR   the built tree whose library and package are used (default: this one)
  --out FILE   where to write (default: tests/golden/solver_traces.json of this tree)"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE.parent))
    ap.add_argument("--out", default=str(HERE.parent / "tests" / "golden" / "solver_traces.json"))
    args = ap.parse_args()
    root = Path(args.root).resolve()
    sys.path[:0] = [str(root / "neptune-pde-solver_amd"), str(HERE.parent / "tests")]
    os.environ["NEPTUNE_HIP_LIB"] = str(root / "neptune-pde-solver_amd" / "lib" / "libneptune_hip.so")
    os.environ.setdefault("NEPTUNE_CACHE_DIR", tempfile.mkdtemp(prefix="neptune_cache_"))
    import torch
    from neptune_hip import _capi, apply, fields, lowering
    import solver_trace_cases as stc

    class NS:
        pass
    nh = NS()
    nh.torch, nh.capi, nh.apply, nh.fields, nh.lowering = torch, _capi, apply, fields, lowering
    _capi.load().neptune_hip_init(0)
    cache, out, failed = {}, {}, []
    for case in stc.cases():
        try:
            out[case[0]] = stc.run(nh, cache, case)
        except AssertionError as e:     # a case that did not take the path it names: report all of them, write nothing
            failed.append(case[0])
            print(case[0], "FAILED", e, flush=True)
            continue
        print(case[0], "rr0", out[case[0]]["rr0"], flush=True)
    if failed:
        raise SystemExit(f"{len(failed)} cases failed: nothing written")
    Path(args.out).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"{len(out)} cases -> {args.out}")


if __name__ == "__main__":
    main()
