"""Monitored applies without a GPU: the lowering option norm-entries.  With it every eligible apply exports
<fn>_<k>__geomN and the report names it as "norm_symbol"; without it source and report do not know the feature exists; the
emitted modules cross-compile for gfx950."""
import json
import subprocess

import pytest

import helpers
import monitor_cases as mc
from make_stencil_mlir import stencil_module

from neptune_hip import lowering


def _fixture(name):
    return (helpers.FIXTURE_DIR / name).read_text()


def _norm_symbols(report):
    return {a["tag"]: a.get("norm_symbol") for a in report["applies"]}


CASES = {
    "apply-3d-7pt": lambda: (_fixture("apply-3d-7pt.mlir"), {"lap3d_0": "lap3d_0__geomN"}),
    "apply-2d-5pt": lambda: (_fixture("apply-2d-5pt.mlir"), {"lap2d_0": "lap2d_0__geomN"}),
    "two-input": lambda: (mc.star_module((9, 12, 256), second_input=True), {"entry_0": "entry_0__geomN"}),
    # @step: time_advance fused with its rhs apply; the opdef's own apply is eligible too
    "fused-euler-step": lambda: (stencil_module("3d7", (9, 12, 256), time_step=0.125),
                                 {"lap3d_0": "lap3d_0__geomN", "step_ta0": "step_ta0__geomN"}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_option_exports_a_norm_entry_per_eligible_apply(name):
    text, want = CASES[name]()
    src, report = lowering.to_hip(text, norm_entries=True)
    got = _norm_symbols(report)
    for tag, sym in want.items():
        assert got[tag] == sym
        assert f'extern "C" int {sym}(const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* sum_out,' in src
        assert f'extern "C" int {sym[:-1]}(' in src          # next to the plain entry, which stays
    assert src.count("neptune_hip::launch_apply_norm<") == len([s for s in got.values() if s])


@pytest.mark.parametrize("name", list(CASES))
def test_without_the_option_source_and_report_do_not_mention_it(name):
    text, _ = CASES[name]()
    src, report = lowering.to_hip(text)
    assert "__geomN" not in src and "launch_apply_norm" not in src
    assert all("norm_symbol" not in a for a in report["applies"])
    # the option line is the only way in: the same text with it is the same module plus the entries
    src_on, report_on = lowering.to_hip(lowering.NORM_ENTRIES_LINE + text)
    assert "__geomN" in src_on and any(a.get("norm_symbol") for a in report_on["applies"])
    assert lowering.to_hip(text, norm_entries=True)[0] == src_on


def test_input0_in_another_box_than_the_result_gets_no_norm_entry():
    text = mc.star_module((9, 12, 256), shifted_input0=True)
    lowering.verify(text)
    src, report = lowering.to_hip(text, norm_entries=True)
    assert report["applies"][0]["geom_symbol"] == "entry_0__geom"
    assert "norm_symbol" not in report["applies"][0] and "__geomN" not in src
    # ... and neither does an input 0 of another element type than the result (there is no such apply to write: the
    # verifier refuses it), so eligibility is the box alone here


def test_norm_entry_modules_cross_compile_for_gfx950(tmp_path, monkeypatch):
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    texts = [stencil_module("3d7", (9, 12, 256), time_step=0.125),      # apply-3d-7pt's operator and a fused Euler @step
             stencil_module("2d5", (24, 512)),                           # apply-2d-5pt's operator
             mc.star_module((9, 12, 256), second_input=True)]
    for text in texts:
        mod_hash = lowering.module_hash(text)
        assert lowering.module_hash(lowering.with_options(text, norm_entries=True)) != mod_hash   # another artefact
        lowering.compile_module(text, load=False, norm_entries=True)
        so = tmp_path / f"neptune_kernel_{lowering.module_hash(lowering.with_options(text, norm_entries=True))}.so"
        assert so.exists()
        report = json.loads(so.with_suffix(".json").read_text())
        syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
        for a in report["applies"]:
            if a.get("norm_symbol"):
                assert f" T {a['norm_symbol']}\n" in syms
        assert any(a.get("norm_symbol") for a in report["applies"])
