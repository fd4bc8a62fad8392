"""The device scalars of cg_solve, cg_solve(minv=...) and bicgstab_solve, bit for bit.

tests/golden/solver_traces.json holds rr_0, every trace row and (with a preconditioner) rz_0 of the solves that
solver_trace_cases.cases() lists, as tools/record_solver_traces.py recorded them.  The replay tests pin the vectors given the
scalars; this pins the scalars themselves, that is the summation tree: per-lane order, the owner of the tail, the order of
the partials, the tree of the one-workgroup kernels.  No oracle work here."""
import json
from pathlib import Path

import pytest

import solver_trace_cases as stc

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "solver_traces.json").read_text())
CASES = stc.cases()


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import os
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache"))
    from neptune_hip import _capi, apply, fields, lowering

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering = torch, _capi, apply, fields, lowering
    _capi.load().neptune_hip_init(0)
    ns.cache = {}
    return ns


def test_the_fixture_holds_exactly_the_listed_cases():
    assert sorted(GOLDEN) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scalars_are_the_recorded_bits(nh, case):
    got, want = stc.run(nh, nh.cache, case), GOLDEN[case[0]]
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k] == want[k], (case[0], k, got[k], want[k])
