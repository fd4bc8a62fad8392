"""Seeded applies of rank 4 to 6 (tests/nd_cases.py) on both lowering paths beyond rank 3, bit for bit against the oracle:
the peeled path (one rank-3 launch per leading index, lowered_runtime.hpp run_apply_batched) on the automatic choice, both
forms of the direct kernel and -- where every sub-slab starts on a 16-byte boundary (nd_cases.tiles_apply) -- every
default rank-3 tile with chunk seams; the rank-generic kernel (kernels/apply_nd.hpp)
on the same settings the runtime offers it; the composed @entry with device and host arguments, fresh and in place.
Then one field per path beyond 2^31 cells, whose last sub-slab starts more than 2^32 bytes into the buffer."""
import os

import numpy as np
import pytest

import helpers
import nd_cases as nc
from helpers import bits_equal, mismatch_report, oracle

pytestmark = pytest.mark.gpu

KNOBS = ("NEPTUNE_HIP_KERNEL", "NEPTUNE_HIP_VARIANT", "NEPTUNE_HIP_CHUNK")


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache_nd_fuzz"))
    from neptune_hip import lowering
    helpers.prefetch_modules([nc.gen_case(seed).text for seed in nc.SEEDS] + [nc.large_text(p) for p in LARGE])
    return lowering, torch


def _set(monkeypatch, s):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in s.items():
        monkeypatch.setenv(k, v)


def _r3(a):
    return a.reshape(-1, *a.shape[-2:])


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_rank4_to_6_applies_match_the_oracle(env, monkeypatch, seed):
    lowering, torch = env
    case = nc.gen_case(seed)
    m = oracle.Module.parse(case.text)
    mod = lowering.compile_module(case.text)
    path = nc.paths(case.text)
    tag = f"seed={seed} rank={case.rank} {case.elem} shape={case.shape}"
    for op in case.ops:
        ins = [helpers.hash_field(case.in_shape(k), case.dtype, seed=seed + 7 * k) for k in range(op.nin)]
        want = m.call(op.name, *ins)
        d_ins = [torch.from_numpy(a).cuda() for a in ins]
        settings = [{}, {"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_KERNEL": "direct-flat"}]
        if path[op.name] == "peeled" and nc.tiles_apply(case):
            settings += [{"NEPTUNE_HIP_KERNEL": "march", "NEPTUNE_HIP_VARIANT": str(v), "NEPTUNE_HIP_CHUNK": str(c)}
                         for v in range(8) for c in (1, 3)]
        for s in settings:
            _set(monkeypatch, s)
            got = mod.call(op.name, *d_ins).cpu().numpy()
            assert bits_equal(got, want), f"{tag} {op.name} path={path[op.name]} bounds={op.bounds} {s}\n" + \
                mismatch_report(_r3(got), _r3(want)) + "\n" + case.text
    # the composed @entry: fresh destination, then in place (destination = input 0), device and host buffers
    _set(monkeypatch, {})
    ins = [helpers.hash_field(case.in_shape(k), case.dtype, seed=seed + 11 * k) for k in range(case.nmax)]
    for inplace in (False, True):
        h_ins = [a.copy() for a in ins]
        h_out = h_ins[0] if inplace else np.full(case.shape, 9.0, dtype=case.dtype)
        m.call("entry", h_out, *h_ins)
        for device in (True, False):
            g_ins = [torch.from_numpy(a.copy()).cuda() if device else a.copy() for a in ins]
            g_out = g_ins[0] if inplace else (torch.full(case.shape, 9.0, dtype=g_ins[0].dtype, device="cuda") if device
                                              else np.full(case.shape, 9.0, dtype=case.dtype))
            mod.call("entry", g_out, *g_ins)
            got = g_out.cpu().numpy() if device else g_out
            assert bits_equal(got, h_out), f"{tag} entry inplace={inplace} device={device} {path}\n" + \
                mismatch_report(_r3(got), _r3(h_out)) + "\n" + case.text


# ---- one rank-4 f32 field per path beyond 2^31 cells (nd_cases.large_text): (3, 1024, 1024, 704) is 2.2e9 cells, 8.9 GB,
# and the sub-slab of leading index 2 starts 5.9 GB into the buffer.  Every cell inside the bounds must be exactly 0, every
# other cell input 0's.
LARGE_SHAPE = nc.LARGE_SHAPE
PEAK_BYTES = 19 * 10 ** 9   # both fields and anything the runtime allocates, below about 20 GB of device memory
LARGE = ("peeled", "nd")


@pytest.mark.parametrize("path", LARGE)
def test_a_rank4_field_beyond_2_pow_31_cells_every_cell(env, monkeypatch, path):
    lowering, torch = env
    _set(monkeypatch, {})
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    mod = lowering.compile_module(nc.large_text(path))
    n0, n1, n2, n3 = LARGE_SHAPE
    assert n0 * n1 * n2 * n3 > 2 ** 31 and 2 * n1 * n2 * n3 * 4 > 2 ** 32
    u = torch.empty(LARGE_SHAPE, dtype=torch.float32, device="cuda")
    out = torch.full(LARGE_SHAPE, float("nan"), dtype=torch.float32, device="cuda")
    try:
        dev = torch.device("cuda")
        lb0, c = nc.LARGE_LB, nc.LARGE_COEF
        ax = [torch.arange(n, dtype=torch.float32, device=dev) + o for n, o in zip(LARGE_SHAPE, lb0)]
        plane = c[2] * ax[2][:, None] + c[3] * ax[3][None, :]                # integers below 2^15: exact in f32
        for a in range(n0):
            for b in range(n1):
                u[a, b] = plane + float(nc.LARGE_COEF0 + c[0] * (a + lb0[0]) + c[1] * (b + lb0[1]))
        mod.call("entry", out, u)
        torch.cuda.synchronize()
        lb, ub = nc.large_bounds(path)
        inner = [slice(a - o, b - o) for a, b, o in zip(lb, ub, nc.LARGE_LB)]
        rim = torch.ones((n2, n3), dtype=torch.bool, device=dev)
        rim[inner[2], inner[3]] = False
        bad_in = bad_rim = 0
        for a in range(n0):
            lead_in = inner[0].start <= a < inner[0].stop
            for b in range(n1):
                row_in = lead_in and inner[1].start <= b < inner[1].stop
                o, x = out[a, b], u[a, b]
                if not row_in:
                    bad_rim += (o.view(torch.int32) != x.view(torch.int32)).sum()
                    continue
                bad_in += (o[inner[2], inner[3]] != 0).sum()
                bad_rim += (o.view(torch.int32)[rim] != x.view(torch.int32)[rim]).sum()
        bad_in, bad_rim = int(bad_in), int(bad_rim)
        assert bad_in == 0 and bad_rim == 0, f"{path}: {bad_in} interior cells not 0, {bad_rim} rim cells not input 0"
        peak = torch.cuda.max_memory_allocated() + pool_bytes()    # torch's tensors, and the runtime's own pool
        assert peak < PEAK_BYTES, peak
        print(f"large {path}: peak device memory {peak / 1e9:.2f} GB")
    finally:
        del u, out
        torch.cuda.empty_cache()


def pool_bytes():
    from neptune_hip import _capi
    return int(_capi.load().neptune_hip_pool_cached_bytes())
