"""Seeded random lowered functions (tests/dataflow_fuzz_cases.py) on the device against the oracle: per seed, function and
argument binding -- all device, all host, mixed, two arguments one device tensor, two arguments one numpy array -- EVERY
argument buffer is bit-equal to the oracle's afterwards on all its cells (untouched arguments and the cells outside every
store box included), an unwrap result is the very object passed in, a temp result is bit-equal and in memory of its own,
and a scalar result is within the tree-height bound of tests/test_reduce_exact_gpu.py.  The two all-device bindings run
once more on the direct kernel: where a result is placed must not depend on the kernel that computes it."""
import math
import os

import numpy as np
import pytest

import dataflow_fuzz_cases as dc
import helpers
import reduce_cases as rc
from helpers import bits_equal, mismatch_report, oracle

pytestmark = pytest.mark.gpu

MODULES = {seed: dc.gen_dataflow_module(seed) for seed in dc.SEEDS}
CASES = [(seed, f["name"], b) for seed in dc.SEEDS for f in MODULES[seed][1]["functions"] for b in dc.BINDINGS]


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache_dataflow"))
    from neptune_hip import lowering
    helpers.prefetch_modules([MODULES[seed][0] for seed in dc.SEEDS])   # every seed's module, compiled side by side
    loaded, parsed = {}, {}

    def get(seed):
        if seed not in loaded:
            loaded[seed] = lowering.compile_module(MODULES[seed][0])
            parsed[seed] = oracle.Module.parse(MODULES[seed][0])
        return loaded[seed], parsed[seed]
    return get, torch


def _span(x):
    if isinstance(x, np.ndarray):
        return x.ctypes.data, x.ctypes.data + x.nbytes
    return x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()


@pytest.mark.parametrize("seed,fn,bname", CASES, ids=[f"{s}-{f}-{b}" for s, f, b in CASES])
def test_every_buffer_and_the_result_match_the_oracle(env, monkeypatch, seed, fn, bname):
    get, torch = env
    text, meta = MODULES[seed]
    mod, m = get(seed)
    f = dc.function(meta, fn)
    bind = next(b for b in dc.bindings(meta, f) if b["name"] == bname)
    want = dc.host_args(meta, f, bind)
    want_res, summed = dc.oracle_run(m, meta, fn, want)
    all_device = set(bind["place"]) == {"d"}
    for setting in [{}] + ([{"NEPTUNE_HIP_KERNEL": "direct"}] if bname in ("device", "aliased-device") else []):
        monkeypatch.delenv("NEPTUNE_HIP_KERNEL", raising=False)
        for k, v in setting.items():
            monkeypatch.setenv(k, v)
        where = f"seed={seed} @{fn} binding={bind} {setting} kinds={f['kinds']}"
        args = [torch.from_numpy(a).cuda() if p == "d" else a for a, p in zip(dc.host_args(meta, f, bind), bind["place"])]
        if bind["alias"]:
            args[bind["alias"][1]] = args[bind["alias"][0]]               # ONE tensor / ONE array under two names
        res = mod.call(fn, *args)
        for k, (a, w) in enumerate(zip(args, want)):
            got = a if isinstance(a, np.ndarray) else a.cpu().numpy()
            assert bits_equal(got, w), f"{where}: argument {k}\n" + mismatch_report(got, w) + "\n" + text
        if f["result"] == "unwrap":
            assert res is args[f["result_arg"]], where
        elif f["result"] == "temp":
            assert isinstance(res, torch.Tensor if all_device else np.ndarray), (where, type(res))
            got = res.cpu().numpy() if all_device else res
            assert bits_equal(got, want_res), f"{where}: result\n" + mismatch_report(got, want_res) + "\n" + text
            lo, hi = _span(res)
            for k, a in enumerate(args):                                  # callee-allocated: none of the arguments' memory
                alo, ahi = _span(a)
                assert hi <= alo or ahi <= lo, f"{where}: the result shares memory with argument {k}"
        elif f["result"] == "scalar":
            x = summed.astype(np.float64).reshape(-1)
            ref, bound = math.fsum(x), rc.gamma(dc.reduce_height(meta, f), meta["dtype"]) * math.fsum(np.abs(x))
            print(f"{where}: scalar {res!r} fsum {ref!r} oracle {want_res!r} |diff| {abs(res - ref):.3e} bound {bound:.3e}")
            assert isinstance(res, float) and abs(res - ref) <= bound, (where, res, ref, bound)
        else:
            assert res is None, where
