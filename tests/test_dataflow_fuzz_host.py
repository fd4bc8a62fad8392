"""The dataflow fuzz cases of tests/dataflow_fuzz_cases.py without a GPU: every function of every seed lowers (none is
skipped or left on the host path), runs in the oracle under each of the five bindings with finite outputs, and the seed
list covers every construct the generator exists for at least twice -- counted from the generator's own record and from
the emitted HIP source, so that a seed list that stops exercising a placement decision fails here."""
import numpy as np
import pytest

import dataflow_fuzz_cases as dc
from helpers import bits_equal, oracle


@pytest.fixture(scope="module")
def lowered():
    from neptune_hip import lowering
    out = {}
    for seed in dc.SEEDS:
        text, meta = dc.gen_dataflow_module(seed)
        src, rep = lowering.to_hip(text)
        out[seed] = (text, meta, src, rep)
    return out


@pytest.mark.parametrize("seed", dc.SEEDS)
def test_the_generator_is_deterministic(seed):
    a, b = dc.gen_dataflow_module(seed), dc.gen_dataflow_module(seed)
    assert a[0] == b[0] and repr(a[1]) == repr(b[1])
    assert a[0] != dc.gen_dataflow_module(seed + 1000)[0]


@pytest.mark.parametrize("seed", dc.SEEDS)
def test_every_function_is_lowered(lowered, seed):
    text, meta, src, rep = lowered[seed]
    names = [name for name, _ in meta["ops"]] + [f["name"] for f in meta["functions"]]
    assert rep["lowered"] == names and not rep.get("skipped"), (seed, rep["lowered"], rep.get("skipped"))
    assert 2 <= len(meta["functions"]) <= 3 and 3 <= len(meta["ops"]) <= 4
    for f in meta["functions"]:
        assert 3 <= len(f["kinds"]) <= 5
    main, wide = meta["boxes"]["main"], meta["boxes"]["wide"]
    assert all(o != 0 for o in main[0])
    assert all(0 <= a - b <= 3 for a, b in zip(main[0], wide[0])) and all(0 <= b - a <= 3 for a, b in zip(main[1], wide[1]))
    assert any(a - b != d - c for (a, b), (c, d) in zip(zip(main[0], wide[0]), zip(main[1], wide[1])))     # asymmetric


@pytest.mark.parametrize("seed", dc.SEEDS)
def test_the_oracle_runs_every_function_under_every_binding(seed):
    text, meta = dc.gen_dataflow_module(seed)
    m = oracle.Module.parse(text)
    for f in meta["functions"]:
        bs = dc.bindings(meta, f)
        assert tuple(b["name"] for b in bs) == dc.BINDINGS
        assert set(bs[2]["place"]) == {"d", "h"} and bs[3]["alias"] == bs[4]["alias"] == f["alias_pair"]
        a, b = f["alias_pair"]
        assert a != b and f["kinds"][a] == f["kinds"][b]
        results = {}
        for bind in bs:
            args = dc.host_args(meta, f, bind)
            assert (args[a] is args[b]) == (bind["alias"] is not None)
            before = [x.copy() for x in args]
            res, summed = dc.oracle_run(m, meta, f["name"], args)         # OutOfBounds / Unsupported would raise here
            for x in args:
                assert np.isfinite(x).all(), (seed, f["name"], bind["name"])
            written = {k for what, k, _ in f["events"] if what == "w"}
            if bind["alias"] and written & {a, b}:
                written |= {a, b}
            for k, (x, x0) in enumerate(zip(args, before)):                   # an argument no store names is left alone
                assert k in written or bits_equal(x, x0), (seed, f["name"], bind["name"], k)
            if f["result"] == "unwrap":
                assert res is args[f["result_arg"]]
            elif f["result"] == "temp":
                assert res.shape == dc.box_shape(meta["boxes"]["main"]) and np.isfinite(res).all()
                assert not any(np.shares_memory(res, x) for x in args)
            elif f["result"] == "scalar":
                assert np.isfinite(res) and summed is not None and dc.reduce_height(meta, f) > 0
            else:
                assert res is None
            results[bind["name"]] = [x.copy() for x in args]
        # where the arguments live does not matter to the oracle: the three distinct bindings agree
        for name in ("host", "mixed"):
            assert all(bits_equal(x, y) for x, y in zip(results["device"], results[name]))


def test_the_seed_list_meets_the_coverage_floors(lowered):
    have = {}
    for seed in dc.SEEDS:
        text, meta, src, rep = lowered[seed]
        for k, v in dc.features(meta, src, rep).items():
            have[k] = have.get(k, 0) + v
    short = {k: (have.get(k, 0), floor) for k, floor in dc.FLOORS.items() if have.get(k, 0) < floor}
    assert not short, short
    assert 10 <= len(dc.SEEDS) <= 14


def test_an_aliased_write_then_read_changes_the_result():
    """the aliased bindings are not the distinct ones over again: over the seed list, binding two arguments to one buffer
    changes what some function computes"""
    differ = 0
    for seed in dc.SEEDS:
        text, meta = dc.gen_dataflow_module(seed)
        m = oracle.Module.parse(text)
        for f in meta["functions"]:
            if not f["alias_write_then_read"]:
                continue
            bs = dc.bindings(meta, f)
            x, y = dc.host_args(meta, f, bs[0]), dc.host_args(meta, f, bs[3])
            dc.oracle_run(m, meta, f["name"], x)
            dc.oracle_run(m, meta, f["name"], y)
            differ += not all(bits_equal(p, q) for p, q in zip(x, y))
    assert differ >= 2
