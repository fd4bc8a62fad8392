"""Every scalar op an apply body may contain, on the device, against the independent model in scalar_spec.py: each op
and type over every value pair of the spec's tables (one case per row, scalar_cases.py), on the march kernel (2-D and
3-D fields) and on both forms of the direct kernel, NaN where the spec says NaN and every other cell bit for bit.  The
elementary functions against a 120-bit reference, in ulps, with C99 Annex F special values exact."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import scalar_cases as SC
import scalar_spec as S

pytestmark = pytest.mark.gpu

# largest error of the device math library over the grids of scalar_cases._grid, in ulps of the correctly rounded
# result: the measured maximum rounded up to a whole ulp
DEVICE_ULP = {
    "f64": {"math.exp": 1, "math.log": 1, "math.sin": 1, "math.cos": 1, "math.tanh": 1, "math.powf": 2},
    "f32": {"math.exp": 1, "math.log": 2, "math.sin": 2, "math.cos": 2, "math.tanh": 1, "math.powf": 2},
}

FAMILIES = [("float", "f64"), ("float", "f32"), ("int", "f64")]
KERNELS = ["march", "direct", "direct-flat"]


def _cases(fam, ty):
    return {"float": SC.float_cases, "int": lambda t: SC.int_cases(), "elem": SC.elementary_cases}[fam](ty)


def _text(fam, ty, rank):
    cases = _cases(fam, ty)
    return SC.module_text(cases, ty, SC.layout(cases, rank))


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache_scalar"))
    from neptune_hip import _capi, lowering
    helpers.prefetch_modules([_text(f, t, r) for f, t in FAMILIES for r in (2, 3)] +
                             [_text("elem", t, 2) for t in ("f64", "f32")])
    return lowering, torch, _capi, _capi.load()


def _run(env, monkeypatch, mod, kernel, ins):
    lowering, torch, capi, lib = env
    for k in ("NEPTUNE_HIP_KERNEL", "NEPTUNE_HIP_VARIANT", "NEPTUNE_HIP_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NEPTUNE_HIP_KERNEL", kernel)
    got = mod.call("ops", *[torch.from_numpy(a).cuda() for a in ins]).cpu().numpy()
    last = capi.LaunchCfg()
    assert lib.neptune_hip_last_launch(C.byref(last)) == 1
    want = capi.KERNEL_MARCH if kernel == "march" else capi.KERNEL_DIRECT
    assert last.kernel == want, f"asked for {kernel}, ran kernel {last.kernel}"      # (the launch record has no form)
    return got


@pytest.mark.parametrize("rank", [2, 3])
@pytest.mark.parametrize("fam,ty", FAMILIES)
def test_every_op_matches_the_spec_on_every_kernel(env, monkeypatch, fam, ty, rank):
    lowering = env[0]
    cases = _cases(fam, ty)
    shape = SC.layout(cases, rank)
    text = SC.module_text(cases, ty, shape)
    mod = lowering.compile_module(text)
    assert [a["kernel"] for a in mod.report["applies"]] == ["march"]       # the automatic choice
    ins, expect = SC.fields(cases, ty, shape)
    report = []
    for kernel in KERNELS:
        got = _run(env, monkeypatch, mod, kernel, ins)
        n, rep = SC.check(got, expect, cases, ty, what=f"{kernel} {shape}: ")
        assert n > 20000
        if rep:
            report.append(rep)
        # the spare last column is the copy-through of input 0
        assert helpers.bits_equal(got[..., -1], ins[0][..., -1])
    assert not report, "\n".join(report)


@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_elementary_functions_against_a_120_bit_reference(env, monkeypatch, ty):
    """ulp error per function within DEVICE_ULP, Annex F special values exact, march and direct kernels bit-identical"""
    pytest.importorskip("mpmath")
    lowering = env[0]
    cases = SC.elementary_cases(ty)
    shape = SC.layout(cases, 2)
    mod = lowering.compile_module(SC.module_text(cases, ty, shape))
    assert mod.report["applies"][0]["exact"] is False
    ins = SC.elementary_fields(cases, ty, shape)
    got = _run(env, monkeypatch, mod, "march", ins)
    for kernel in ("direct", "direct-flat"):
        other = _run(env, monkeypatch, mod, kernel, ins)
        assert helpers.bits_equal(other, got), f"{kernel} vs march: " + helpers.mismatch_report(other, got)
    worst, bad = SC.elementary_check(got, cases, ty, shape)
    print(f"device {ty} max ulp error: " + ", ".join(f"{f} {w:.3f}" for f, w in worst.items()))
    assert not bad, "\n".join(bad)
    over = {f: w for f, w in worst.items() if w > DEVICE_ULP[ty][f]}
    assert not over, f"device {ty}: ulp error above the bound: {over} (bounds {DEVICE_ULP[ty]})"
