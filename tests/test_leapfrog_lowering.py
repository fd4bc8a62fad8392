"""Lowering of two-level (leapfrog) steps: an apply whose input 0 is a star of radius <= 2 and whose other inputs are read at
the centre only exports <tag>__geomL2 -- two steps per pass over HBM, both states stored (csrc/kernels/apply_march2.hpp) --
next to <tag>__geom, and the report names it as "leapfrog_symbol".  No GPU needed: hipcc cross-compiles."""
import re

import pytest

import helpers
import leapfrog_cases as lc


@pytest.fixture(autouse=True)
def _built(built_libs):
    pass


def wave_apply(report):
    (a,) = [a for a in report["applies"] if a["function"] == "wave"]
    return a


@pytest.mark.parametrize("shape,radius,coef", [((16, 24, 128), 1, False), ((16, 24, 128), 1, True), ((16, 24, 128), 2, False),
                                               ((40, 256), 1, False), ((40, 256), 2, True)])
def test_a_two_level_step_gets_a_pair_entry(shape, radius, coef):
    from neptune_hip import lowering
    src, report = lowering.to_hip(lc.module_text(shape, radius=radius, coef=coef))
    a = wave_apply(report)
    assert a["geom_symbol"] == "wave_0__geom" and a["leapfrog_symbol"] == "wave_0__geomL2"
    assert 'extern "C" int wave_0__geomL2(const neptune_hip_apply_geom_t* g, const void* const* in, void* out_v, void* out_w,' in src
    nin = 3 if coef else 2
    assert f"neptune_hip::launch_apply_leapfrog2<Body_wave_0, double, {len(shape)}, {nin}, FP_wave_0>" in src
    # the ordinary entries are still there, once each
    for suffix in ("", "2", "3"):
        assert len(re.findall(rf'extern "C" int wave_0__geom{suffix}\(', src)) == 1


def test_previous_state_read_at_an_offset_is_not_a_leapfrog_step():
    from neptune_hip import lowering
    src, report = lowering.to_hip(lc.module_text((16, 24, 128), prev_offset=[0, 0, 1]))
    a = wave_apply(report)
    assert a["geom_symbol"] == "wave_0__geom" and a["leapfrog_symbol"] == ""
    assert "__geomL2" not in src and "launch_apply_leapfrog2" not in src


def test_a_single_input_apply_has_no_pair_entry():
    from neptune_hip import lowering
    src, report = lowering.to_hip(lc.single_input_text((16, 24, 128)))
    assert [a["leapfrog_symbol"] for a in report["applies"]] == [""] * len(report["applies"])
    assert any(a["geom_symbol"] for a in report["applies"])
    assert "__geomL2" not in src


def test_a_radius_3_star_has_no_pair_entry():
    from neptune_hip import lowering
    src, report = lowering.to_hip(lc.module_text((16, 24, 128), radius=3))
    a = wave_apply(report)
    assert a["geom_symbol"] == "wave_0__geom" and a["kernel"] == "march" and a["leapfrog_symbol"] == ""
    assert "__geomL2" not in src


def test_every_report_entry_carries_the_key():
    from neptune_hip import lowering
    _, report = lowering.to_hip(helpers.stencil_module("3d7", [10, 36, 256], time_step=0.125))
    assert report["applies"] and all(a["leapfrog_symbol"] == "" for a in report["applies"])


@pytest.mark.parametrize("shape,elem,radius,coef", [((16, 24, 128), "f64", 1, True), ((16, 24, 128), "f32", 2, False),
                                                    ((40, 256), "f64", 2, True)])
def test_qualifying_modules_compile_for_gfx950(shape, elem, radius, coef, tmp_path, monkeypatch):
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    from neptune_hip import lowering
    mod = lowering.compile_module(lc.module_text(shape, elem=elem, radius=radius, coef=coef))
    entry = mod.geom_entry("wave")
    assert entry.fn_leapfrog2 is not None and entry.fn is not None
    # an apply that does not qualify: GeomEntry says so with None
    plain = lowering.compile_module(lc.module_text(shape, elem=elem, radius=radius, coef=coef, prev_offset=[0] * (len(shape) - 1) + [1]))
    assert plain.geom_entry("wave").fn_leapfrog2 is None


def test_header_and_bindings_name_the_loop():
    from neptune_hip import _capi
    header = (helpers.REPO / "include/neptune_hip.h").read_text()
    for name in ("neptune_hip_step_loop_leapfrog", "neptune_hip_leapfrog_launch_counts"):
        assert name in header and name in _capi.SIGNATURES
    assert "neptune_hip_leapfrog2_fn" in header
    lib = _capi.load()
    assert lib.neptune_hip_step_loop_leapfrog is not None
