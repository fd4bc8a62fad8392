"""Groups of sibling applies over shared inputs run as ONE multi-output launch: every result field of the two
system fixtures (tests/mlir_tests/systems) and of their size variants is bit-identical to the oracle -- on the automatic
tile, on every march tile, on both direct forms, with apply.bounds strictly inside the box (a different copy-through
source per member), with a destination that aliases another member's input, and where the group must fall back to one
launch per member.  Only IEEE-exact operations: no tolerance anywhere."""
import os

import numpy as np
import pytest

import group_cases as gc
import helpers
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

ENV_KEYS = ("NEPTUNE_HIP_KERNEL", "NEPTUNE_HIP_VARIANT", "NEPTUNE_HIP_CHUNK", "NEPTUNE_HIP_NO_GROUPS")
# (kind, shape): one small, one whose rows are not a whole number of lane vectors (f64: 2 cells, f32: 4)
SMALL = [("swe", (40, 512)), ("swe", (37, 515)), ("pair", (13, 19, 256)), ("pair", (11, 18, 261))]
PRODUCTION = {"swe": (8192, 8192), "pair": (512, 512, 512)}
ELEMS = {"f64": np.float64, "f32": np.float32}


def inner_bounds(shape):
    """apply.bounds strictly inside the box, unevenly: copy-through layers of different thickness on every side"""
    return [2] + [1] * (len(shape) - 1), [shape[0] - 3] + [n - 2 for n in shape[1:]]


def radius2_pair(shape):
    """two radius-2 members in 3-D: the union footprint (two inputs read at wide offsets) is planned onto the plane-in-LDS
    kernel, which has no group form"""
    text = gc.variant("pair", shape, [2, 2, 2], [n - 2 for n in shape])
    for a, b in (("[-1, 0, 0]", "[-2, 0, 0]"), ("[1, 0, 0]", "[2, 0, 0]"), ("[0, -1, 0]", "[0, -2, 0]"), ("[0, 1, 0]", "[0, 2, 0]"),
                 ("[0, 0, -1]", "[0, 0, -2]"), ("[0, 0, 1]", "[0, 0, 2]")):
        assert text.count(a) == 2
        text = text.replace(a, b)
    # both members read BOTH fields at radius 2: %w becomes a neighbour of the other field
    assert text.count("%o[0, 0, 0]") == 2
    return text.replace("%o[0, 0, 0]", "%o[0, -2, 0]")


def all_texts():
    out = [gc.variant(k, s, *inner_bounds(s), elem=e) for k, s in SMALL for e in ELEMS]
    out += [gc.variant(k, s, elem=e) for k, s in PRODUCTION.items() for e in ELEMS]
    out += [gc.variant("swe", (24, 512)), radius2_pair((12, 20, 256))]
    return out


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    # a cache filled beforehand (same build) saves the compiles; otherwise they run side by side here
    os.environ["NEPTUNE_CACHE_DIR"] = os.environ.get("NEPTUNE_GROUP_TEST_CACHE") or str(tmp_path_factory.mktemp("neptune_cache_grp"))
    import neptune_hip as nh
    from neptune_hip import apply, lowering  # noqa: F401  (nh.apply: the group launch counters)
    helpers.prefetch_modules(all_texts())
    return lowering, torch, nh


@pytest.fixture
def launch_env():
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def set_env(setting):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(setting)


def run(mod, torch, shape, dtype, ins, fill=-7.0):
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    d_ins = [torch.from_numpy(a).cuda() for a in ins]
    d_outs = [torch.full(shape, fill, dtype=tdt, device="cuda") for _ in ins]
    mod.call("entry", *d_outs, *d_ins)
    torch.cuda.synchronize()
    return d_outs


@pytest.mark.parametrize("elem", list(ELEMS))
@pytest.mark.parametrize("kind,shape", SMALL, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in SMALL])
def test_group_matches_the_oracle_on_every_tile_and_direct_form(env, launch_env, kind, shape, elem):
    lowering, torch, nh = env
    dtype = ELEMS[elem]
    lb, ub = inner_bounds(shape)
    text = gc.variant(kind, shape, lb, ub, elem)
    ins = gc.inputs(kind, shape, dtype)
    want = gc.oracle_run(text, shape, dtype, ins)
    mod = lowering.compile_module(text)
    assert len(mod.report["groups"]) == 1 and mod.report["groups"][0]["kernel"] == "march"
    nvar = {3: 8, 2: 3}[len(shape)]
    settings = [{}] + [{"NEPTUNE_HIP_VARIANT": str(v), "NEPTUNE_HIP_CHUNK": c} for v in range(nvar) for c in ("1", "4")]
    settings += [{"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_KERNEL": "direct-flat"}, {"NEPTUNE_HIP_NO_GROUPS": "1"}]
    n = gc.NOUT[kind]
    for s in settings:
        set_env(s)
        before = nh.apply.group_launch_counts()
        outs = run(mod, torch, shape, dtype, ins)
        after = nh.apply.group_launch_counts()
        # ONE launch for the group; with NEPTUNE_HIP_NO_GROUPS=1 one per member
        assert (after[0] - before[0], after[1] - before[1]) == ((0, n) if "NEPTUNE_HIP_NO_GROUPS" in s else (1, 0)), s
        for m in range(n):
            got = outs[m].cpu().numpy()
            assert bits_equal(got, want[m]), f"{kind} {shape} {elem} {s} result {m}: " + mismatch_report(got, want[m])
    # outside apply.bounds member m's result is member m's OWN unknown
    for m in range(n):
        assert bits_equal(want[m][:2], ins[m][:2]) and bits_equal(want[m][-3:], ins[m][-3:])


@pytest.mark.parametrize("elem", list(ELEMS))
@pytest.mark.parametrize("kind", list(PRODUCTION))
def test_production_size_group_equals_the_member_launches_and_the_oracle(env, launch_env, kind, elem):
    lowering, torch, nh = env
    dtype, shape = ELEMS[elem], PRODUCTION[kind]
    lb, ub = [1] * len(shape), [n - 1 for n in shape]
    mod = lowering.compile_module(gc.variant(kind, shape, elem=elem))
    ins = gc.inputs(kind, shape, dtype)
    set_env({})
    before = nh.apply.group_launch_counts()
    grouped = run(mod, torch, shape, dtype, ins)
    assert nh.apply.group_launch_counts()[0] == before[0] + 1        # the automatic plan fuses both fixtures
    set_env({"NEPTUNE_HIP_NO_GROUPS": "1"})
    single = run(mod, torch, shape, dtype, ins)
    it = torch.int64 if dtype == np.float64 else torch.int32
    for m, (a, b) in enumerate(zip(grouped, single)):
        assert torch.equal(a.view(it), b.view(it)), f"{kind} {elem}: result {m} differs between the group and the member launches"
    # sampled rows / planes against the oracle: both boundaries, around the usual chunk seams, the middle
    n0 = shape[0]
    for g0 in (0, 30, 62, 126, 254, n0 // 2 - 2, n0 - 130, n0 - 4):
        g1 = g0 + 4
        want = gc.oracle_band(kind, shape, lb, ub, dtype, ins, g0, g1)
        for m in range(gc.NOUT[kind]):
            got = grouped[m][g0:g1].cpu().numpy()
            assert bits_equal(got, np.ascontiguousarray(want[m])), f"{kind} {elem} rows {g0}:{g1} result {m}: " + mismatch_report(got, np.ascontiguousarray(want[m]))


def test_a_destination_that_aliases_another_members_input_gets_a_temporary(env, launch_env):
    """in-place update of h while the momentum members still read h: the oracle gives every apply a private result and
    stores afterwards; the group does the same for that member and still fuses the launch"""
    lowering, torch, nh = env
    shape = (24, 512)
    text = gc.variant("swe", shape)
    h, qx, qy = gc.inputs("swe", shape, np.float64)
    want = gc.oracle_run(text, shape, np.float64, [h, qx, qy])
    h_inplace, oqx, oqy = h.copy(), np.zeros_like(h), np.zeros_like(h)
    helpers.oracle.Module.parse(text).call("entry", h_inplace, oqx, oqy, h_inplace, qx, qy)
    assert bits_equal(h_inplace, want[0]) and bits_equal(oqx, want[1]) and bits_equal(oqy, want[2])
    mod = lowering.compile_module(text)
    for s in ({}, {"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_NO_GROUPS": "1"}):
        set_env(s)
        d_h, d_qx, d_qy = (torch.from_numpy(a).cuda() for a in (h, qx, qy))
        d_oqx, d_oqy = torch.zeros_like(d_h), torch.zeros_like(d_h)
        mod.call("entry", d_h, d_oqx, d_oqy, d_h, d_qx, d_qy)
        torch.cuda.synchronize()
        for m, t in enumerate((d_h, d_oqx, d_oqy)):
            got = t.cpu().numpy()
            assert bits_equal(got, want[m]), f"{s} result {m}: " + mismatch_report(got, want[m])


def test_a_group_without_a_group_form_runs_member_by_member(env, launch_env):
    lowering, torch, nh = env
    shape = (12, 20, 256)
    text = radius2_pair(shape)
    mod = lowering.compile_module(text)
    assert len(mod.report["groups"]) == 1 and mod.report["groups"][0]["kernel"] == "members"
    ins = gc.inputs("pair", shape, np.float64)
    want = gc.oracle_run(text, shape, np.float64, ins)
    set_env({})
    before = nh.apply.group_launch_counts()
    outs = run(mod, torch, shape, np.float64, ins)
    after = nh.apply.group_launch_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (0, 2)
    for m in range(2):
        got = outs[m].cpu().numpy()
        assert bits_equal(got, want[m]), f"result {m}: " + mismatch_report(got, want[m])
