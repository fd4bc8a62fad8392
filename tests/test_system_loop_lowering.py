"""A group's geometry-level entry (<fn>_<k0>_group__geom) and the system step loop built on it, without a GPU: what the
lowering emits and reports, that the module cross-compiles for gfx950 with the symbol in it, that header, library and
Python prototypes agree, and that the inputs the GPU tests step stay finite on the oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import group_cases as gc
import helpers
import system_loop_cases as sc
from test_group_gpu import radius2_pair

from neptune_hip import _capi, lowering

ENTRY = 'extern "C" int entry_0_group__geom('


@pytest.mark.parametrize("kind", ["swe", "pair"])
def test_fixture_exports_one_group_entry_and_reports_it(kind, tmp_path, monkeypatch):
    src, report = lowering.to_hip(gc.fixture_text(kind))
    assert src.count(ENTRY) == 1
    # through the launchers, not through the lowered function's wrappers, and once: the entry instantiates what the
    # lowered function already holds
    assert src.count("neptune_hip::apply_group_geom<Group_entry_0_group,") == 1
    assert src.count("nl::run_apply_group<") == 1 and "nl::run_apply<" not in src
    grp = report["groups"][0]
    assert grp["geom_symbol"] == "entry_0_group__geom"
    assert grp["rank"] == (2 if kind == "swe" else 3) and grp["elem"] == "f64"
    assert grp["through"] == sc.THROUGH[kind]
    # `through` is each member's input 0 among the union inputs
    assert grp["through"] == [m[0] for m in sc.MEMBER_INPUTS[kind]]
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    mod = lowering.compile_module(gc.variant(kind, sc.LOOP_SMALL[kind]))      # hipcc --offload-arch=gfx950; no device needed
    assert hasattr(mod.lib, "entry_0_group__geom")
    entry = mod.group_entry("entry")
    assert entry.symbol == "entry_0_group__geom" and entry.through == sc.THROUGH[kind]
    assert entry.num_outputs == gc.NOUT[kind] and entry.num_inputs == gc.NOUT[kind]
    assert entry.rank == len(sc.LOOP_SMALL[kind]) and entry.dtype == _capi.F64
    assert entry.inputs == (["%h", "%qx", "%qy"] if kind == "swe" else ["%u", "%v"])
    with pytest.raises(KeyError):
        mod.group_entry("entry", 1)


def test_a_group_without_a_group_form_still_gets_an_entry():
    src, report = lowering.to_hip(radius2_pair((12, 20, 256)))
    grp = report["groups"][0]
    assert grp["kernel"] == "members" and grp["geom_symbol"] == "entry_0_group__geom" and grp["through"] == [0, 1]
    assert src.count(ENTRY) == 1


def test_a_fixed_input_is_nobodys_unknown():
    text = sc.fixed_input_variant((24, 64))
    lowering.verify(text)
    src, report = lowering.to_hip(text)
    grp = report["groups"][0]
    assert grp["inputs"] == ["%h", "%qx", "%qy", "%b"] and grp["through"] == [0, 1, 2] and len(grp["members"]) == 3
    assert src.count(ENTRY) == 1


def test_a_module_without_a_group_emits_no_group_entry():
    src, report = lowering.to_hip(helpers.stencil_module("3d7", (16, 16, 64)))
    assert report["groups"] == [] and "_group__geom" not in src and "apply_group_geom" not in src


def test_header_library_and_prototypes_hold_the_two_functions():
    header = _capi.HEADER_PATH.read_text()
    assert re.search(r"\bint neptune_hip_step_loop_system\(neptune_hip_group_fn fn,", header)
    assert re.search(r"\bvoid neptune_hip_system_loop_counts\(int64_t \*launches, int64_t \*graph_launches\);", header)
    assert "typedef int (*neptune_hip_group_fn)(" in header
    lib = C.CDLL(str(_capi.library_path()))
    for name in ("neptune_hip_step_loop_system", "neptune_hip_system_loop_counts"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES


@pytest.mark.parametrize("elem", list(sc.ELEMS))
def test_loop_inputs_stay_finite_on_the_oracle(elem):
    """what the GPU tests step: bounded well away from a division by zero, so no NaN (whose sign differs between
    processors) can enter a bit-exact comparison"""
    dtype = sc.ELEMS[elem]
    shape = sc.LOOP_SMALL["swe"]
    states = sc.oracle_states(gc.variant("swe", shape, elem=elem), sc.loop_inputs("swe", shape, dtype), 50)
    assert all(np.isfinite(a).all() for s in states for a in s)
    assert min(s[0].min() for s in states) > 0.9 and max(s[0].max() for s in states) < 1.15
    fixed = sc.fixed_field(shape, dtype)
    states = sc.oracle_states(sc.fixed_input_variant(shape, elem), sc.loop_inputs("swe", shape, dtype), 50, [fixed])
    assert all(np.isfinite(a).all() for s in states for a in s)
    assert min(s[0].min() for s in states) > 0.9 and max(s[0].max() for s in states) < 1.15
    # the fixed field really enters: the first step differs from the plain fixture's by nu * b inside apply.bounds
    plain = sc.oracle_states(gc.variant("swe", shape, elem=elem), sc.loop_inputs("swe", shape, dtype), 1)
    assert not helpers.bits_equal(states[1][0], plain[1][0]) and helpers.bits_equal(states[1][1], plain[1][1])
    shape = sc.LOOP_SMALL["pair"]
    states = sc.oracle_states(gc.variant("pair", shape, elem=elem), sc.loop_inputs("pair", shape, dtype), 50)
    assert all(np.isfinite(a).all() and np.abs(a).max() < 1.25 for s in states for a in s)
