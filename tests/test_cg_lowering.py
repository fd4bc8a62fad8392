"""Dot-monitored applies without a GPU: the lowering option dot-entries.  With it every apply that is eligible
under the norm-entries rule exports <fn>_<k>__geomD and the report names it as "dot_symbol"; without it source and report are
byte for byte what they are without the feature; neptune-opt takes --dot-entries; the emitted modules cross-compile for gfx950."""
import json
import subprocess

import numpy as np
import pytest

import cg_cases as cc
import helpers
import monitor_cases as mc
from make_stencil_mlir import stencil_module

from neptune_hip import _capi, lowering

NEPTUNE_OPT = _capi.PKG_ROOT / "bin" / "neptune-opt"


def _fixture(name):
    return (helpers.FIXTURE_DIR / name).read_text()


CASES = {
    "apply-3d-7pt": lambda: (_fixture("apply-3d-7pt.mlir"), {"lap3d_0": "lap3d_0__geomD"}),
    "apply-2d-5pt": lambda: (_fixture("apply-2d-5pt.mlir"), {"lap2d_0": "lap2d_0__geomD"}),
    "cg-operator": lambda: (cc.cg_module((9, 11, 131)), {"entry_0": "entry_0__geomD"}),
    "two-input": lambda: (mc.star_module((9, 12, 256), second_input=True), {"entry_0": "entry_0__geomD"}),
    "fused-euler-step": lambda: (stencil_module("3d7", (9, 12, 256), time_step=0.125),
                                 {"lap3d_0": "lap3d_0__geomD", "step_ta0": "step_ta0__geomD"}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_option_exports_a_dot_entry_per_eligible_apply(name):
    text, want = CASES[name]()
    src, report = lowering.to_hip(text, dot_entries=True)
    assert lowering.DOT_ENTRIES_LINE == "// neptune-hip-option: dot-entries\n"
    got = {a["tag"]: a.get("dot_symbol") for a in report["applies"]}
    for tag, sym in want.items():
        assert got[tag] == sym
        assert f'extern "C" int {sym}(const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* dot_out,' in src
        assert f'extern "C" int {sym[:-1]}(' in src          # next to the plain entry, which stays
    assert src.count("neptune_hip::launch_apply_dot<") == len([s for s in got.values() if s])
    assert "launch_apply_norm" not in src and all("norm_symbol" not in a for a in report["applies"])   # its own option


@pytest.mark.parametrize("name", list(CASES))
def test_without_the_option_source_and_report_are_untouched(name):
    text, _ = CASES[name]()
    src, report = lowering.to_hip(text)
    assert "__geomD" not in src and "launch_apply_dot" not in src and "dot_out" not in src
    assert all("dot_symbol" not in a for a in report["applies"])
    # the option line is the only way in, and it only ADDS the entries: removing them gives back the default source
    src_on, report_on = lowering.to_hip(lowering.DOT_ENTRIES_LINE + text)
    assert lowering.to_hip(text, dot_entries=True) == (src_on, report_on)
    kept, skipping = [], False
    for line in src_on.splitlines(keepends=True):
        if line.startswith("// the dot-monitored launch"):
            skipping = True
        if skipping and line.startswith("// march tiles this module holds"):
            skipping = False
        if not skipping:
            kept.append(line)
    # (against the text with a comment line in the option line's place: the source quotes line numbers; the module id is a
    # hash of the text)
    module_id = lambda t: [ln for ln in t.splitlines() if "NEPTUNE_HIP_MODULE_ID" not in ln]
    assert module_id("".join(kept)) == module_id(lowering.to_hip("// no option here\n" + text)[0])
    for a in report_on["applies"]:
        a.pop("dot_symbol", None)
    assert report_on == report
    # both options together: both entries
    src_both, report_both = lowering.to_hip(text, norm_entries=True, dot_entries=True)
    assert all(bool(a.get("norm_symbol")) == bool(a.get("dot_symbol")) for a in report_both["applies"])
    assert src_both.count("launch_apply_norm<") == src_both.count("launch_apply_dot<") >= 1


def test_input0_in_another_box_than_the_result_gets_no_dot_entry():
    text = mc.star_module((9, 12, 256), shifted_input0=True)
    src, report = lowering.to_hip(text, dot_entries=True)
    assert report["applies"][0]["geom_symbol"] == "entry_0__geom"
    assert "dot_symbol" not in report["applies"][0] and "__geomD" not in src


def test_command_line_option(built_libs, tmp_path):
    if not NEPTUNE_OPT.exists():
        subprocess.run(["make", "-C", str(_capi.REPO_ROOT), "lowering"], check=True)
    text = cc.cg_module((9, 11, 131))
    path = tmp_path / "op.mlir"
    path.write_text(text)
    run = lambda *flags: subprocess.run([str(NEPTUNE_OPT), str(path), "--neptuneir-to-hip", "--report", *flags], check=True,
                                        capture_output=True, text=True)
    on, off = run("--dot-entries"), run()
    assert on.stdout == lowering.to_hip(text, dot_entries=True)[0]
    assert json.loads(on.stderr)["applies"][0]["dot_symbol"] == "entry_0__geomD"
    assert off.stdout == lowering.to_hip(text)[0] and "dot_symbol" not in off.stderr


def test_dot_entry_modules_cross_compile_for_gfx950(tmp_path, monkeypatch):
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    texts = [cc.cg_module((9, 11, 131)),                                 # the solver tests' operator
             cc.cg_module((12, 20, 136), np.float32, radius=2),          # its radius-2 variant, f32
             stencil_module("2d5", (24, 512))]
    for text in texts:
        with_opt = lowering.with_options(text, dot_entries=True)
        assert lowering.module_hash(with_opt) != lowering.module_hash(text)   # another artefact
        lowering.compile_module(text, load=False, dot_entries=True)
        so = tmp_path / f"neptune_kernel_{lowering.module_hash(with_opt)}.so"
        assert so.exists()
        report = json.loads(so.with_suffix(".json").read_text())
        syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
        assert any(a.get("dot_symbol") for a in report["applies"])
        for a in report["applies"]:
            if a.get("dot_symbol"):
                assert f" T {a['dot_symbol']}\n" in syms



def test_solver_and_dot_refuse_bad_arguments_before_touching_a_device(built_libs):
    """the argument checks of neptune_hip_cg_solve / neptune_hip_dot / neptune_hip_apply_builtin_dot run before the device is
    initialised: NEPTUNE_HIP_EINVAL on host buffers, on a box without a GPU"""
    import ctypes as C
    from neptune_hip.geometry import make_geom
    lib = _capi.load()
    shape = (4, 5, 8)
    n = 4 * 5 * 8
    bufs = [(C.c_double * (n + 8))() for _ in range(5)]
    x, b, r, p, q = [C.addressof(a) for a in bufs]
    box = ([0, 0, 0], list(shape))
    g = make_geom(box, ([1, 1, 1], [3, 4, 7]), [box], None)
    done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)

    def solve(xp=x, bp=b, w=(r, p, q), max_iters=4, check_every=1, trace=None, geom=g, body=_capi.BODY_LAP3D7_F64):
        return lib.neptune_hip_cg_solve(None, None, body, _capi.F64, C.byref(geom), xp, bp, (C.c_void_p * 3)(*w), None, max_iters,
                                        check_every, 0.0, trace, None, None, C.byref(done), C.byref(rr0), C.byref(last))
    E = _capi.EINVAL
    assert solve(check_every=0) == E and solve(max_iters=-1) == E
    assert solve(xp=None) == E and solve(bp=None) == E and solve(w=(r, None, q)) == E
    assert solve(bp=x) == E and solve(w=(r, r + 8 * (n - 1), q)) == E and solve(w=(r, p, x + 8)) == E
    assert solve(trace=p + 16) == E                                      # a trace inside p
    assert solve(body=99) == E
    shifted = make_geom(box, ([1, 1, 1], [3, 4, 7]), [([1, 0, 0], [5, 5, 8])], None)
    assert solve(geom=shifted) == E                                      # input 0 in another box than the result
    assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
    assert lib.neptune_hip_dot(_capi.F64, C.byref(g), None, b, r, None) == E
    assert lib.neptune_hip_dot(7, C.byref(g), x, b, r, None) == E
    assert lib.neptune_hip_apply_builtin_dot(99, C.byref(g), (C.c_void_p * 1)(x), b, r, None, None) == E
    assert lib.neptune_hip_apply_builtin_dot(_capi.BODY_LAP3D7_F64, C.byref(g), (C.c_void_p * 1)(x), x, r, None, None) == E   # out == in
