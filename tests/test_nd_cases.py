"""The rank-4..6 cases of tests/nd_cases.py without a GPU: every seed lowers onto the path it was meant for and runs in
the oracle, the seed list meets its coverage quotas, and the oracle itself passes a metamorphic check -- a peeled apply at
one leading index is the rank-3 apply of the same body with that index as constants, on the rank-3 slices of its inputs,
and outside the leading bounds it is input 0's slice."""
import numpy as np
import pytest

import helpers
import nd_cases as nc
from helpers import bits_equal, mismatch_report, oracle

REQUIRED = ({f"rank{r}-{e}" for r in (4, 5, 6) for e in ("f64", "f32")}
            | {f"{p}-rank{r}" for p in ("peeled", "nd") for r in (4, 5, 6)}
            | {f"{p}-{m}" for p in ("peeled", "nd") for m in ("full", "cut", "empty-lead")}
            | {f"peeled-lead-index-{d}" for d in range(3)} | {f"nd-lead-index-{d}" for d in range(3)}
            | {f"nin{n}" for n in range(1, 5)}
            | {"lead-extent-1", "lead-extent-1-beside-5", "ragged", "aligned", "store-full", "store-box",
               "peeled-lead-cut", "tiles", "tiles-ragged", "slab-misaligned", "nd-lead-cut", "peeled-lead-margin", "peeled-inner-lead-margin", "nd-lead-margin"})


def inputs(case, n, salt=7):
    return [helpers.hash_field(case.in_shape(k), case.dtype, seed=case.seed + salt * k) for k in range(n)]


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_every_seed_lowers_onto_the_path_it_was_meant_for(seed):
    from neptune_hip import lowering
    case = nc.gen_case(seed)
    assert 4 <= case.rank <= 6 and len(case.boxes) == case.nmax
    for k in range(1, case.nmax):                    # inputs 1.. contain the result's box
        assert all(a <= b for a, b in zip(case.boxes[k][0], case.boxes[0][0]))
        assert all(a >= b for a, b in zip(case.boxes[k][1], case.boxes[0][1]))
    got = nc.paths(case.text)
    assert got == {op.name: op.kind for op in case.ops}, (seed, got)
    _, rep = lowering.to_hip(case.text)
    assert rep["lowered"] == [op.name for op in case.ops] + ["entry"] and not rep.get("skipped")
    kern = {a["function"]: a["kernel"] for a in rep["applies"]}
    for op in case.ops:                              # a peeled apply runs the rank-3 march kernel: every tile applies
        assert kern[op.name] == ("march" if op.kind == "peeled" else "direct"), (seed, op.name, kern)
    for op in case.ops:
        assert op.kind == "peeled" or any(any(off[:case.lead]) for _, off in op.accesses)
        assert op.kind == "nd" or not any(any(off[:case.lead]) for _, off in op.accesses)
    assert all(n * np.dtype(case.dtype).itemsize < 64 << 20 for n in (int(np.prod(case.in_shape(k))) for k in range(case.nmax)))


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_every_seed_runs_in_the_oracle(seed):
    case = nc.gen_case(seed)
    m = oracle.Module.parse(case.text)
    for op in case.ops:
        ins = inputs(case, op.nin)
        got = m.call(op.name, *ins)
        assert got.shape == case.shape and got.dtype == case.dtype
        if op.bounds_mode == "empty-lead":
            assert bits_equal(got, ins[0])
        else:
            assert not bits_equal(got, ins[0])
    ins = inputs(case, case.nmax, salt=11)
    out = np.full(case.shape, 9.0, dtype=case.dtype)
    assert m.call("entry", out, *ins) is out
    if case.store is not None:                       # cells outside the stored box keep the destination's value
        keep = np.ones(case.shape, bool)
        keep[tuple(slice(a - o, b - o) for a, b, o in zip(case.store[0], case.store[1], case.boxes[0][0]))] = False
        assert keep.any() and (out[keep] == 9.0).all()


def test_the_seed_list_meets_the_coverage_quotas():
    seen = set()
    for seed in nc.SEEDS:
        seen |= nc.features(nc.gen_case(seed))
    assert not REQUIRED - seen, sorted(REQUIRED - seen)
    assert 12 <= len(nc.SEEDS) <= 16


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_a_peeled_apply_is_the_rank3_apply_at_each_leading_index(seed):
    """metamorphic check of the oracle: the rank-R result at leading index j equals the rank-3 opdef with the leading index
    arguments replaced by j, run on the rank-3 slices of the inputs; outside the leading bounds it is input 0's slice"""
    case = nc.gen_case(seed)
    m = oracle.Module.parse(case.text)
    op = next(o for o in case.ops if o.kind == "peeled")
    ins = inputs(case, op.nin)
    full = m.call(op.name, *ins)
    n_in = n_out = 0
    for j in nc.lead_indices(case):
        got = full[nc.lead_slice(case, 0, j)]
        if not nc.inside_lead(op, j):
            assert bits_equal(got, ins[0][nc.lead_slice(case, 0, j)]), (seed, j)
            n_out += 1
            continue
        sl = [np.ascontiguousarray(ins[k][nc.lead_slice(case, k, j)]) for k in range(op.nin)]
        want = oracle.Module.parse(nc.slice_module(case, op, j)).call("op", *sl)
        assert bits_equal(got, want), f"seed={seed} lead={j}\n" + mismatch_report(got, want)
        n_in += 1
    assert n_in + n_out == int(np.prod(case.shape[:case.lead]))
    assert n_in > 0 or op.bounds_mode == "empty-lead"


@pytest.mark.parametrize("path", ["peeled", "nd"])
def test_the_large_cases_take_their_paths_and_are_exact_in_the_oracle(path):
    """the bodies of test_nd_fuzz_gpu's fields beyond 2^31 cells, on a small box of the same form: the lowering picks the
    path, and the oracle gives exactly 0 inside the bounds and input 0 elsewhere"""
    assert nc.paths(nc.large_text(path)) == {"lap": path}
    shape = (3, 6, 5, 9)
    u = nc.large_affine(shape)
    corners = [abs(nc.LARGE_COEF0) + sum(c * max(abs(o), abs(o + n - 1)) for c, o, n in zip(nc.LARGE_COEF, nc.LARGE_LB, nc.LARGE_SHAPE))]
    assert corners[0] * 9 < 2 ** 24          # every value and partial sum of the body is an exact f32 integer
    got = oracle.Module.parse(nc.large_text(path, shape)).call("lap", u)
    lb, ub = nc.large_bounds(path, shape)
    want = u.copy()
    want[tuple(slice(a - o, b - o) for a, b, o in zip(lb, ub, nc.LARGE_LB))] = 0
    assert bits_equal(got, want), mismatch_report(got, want)
    assert not bits_equal(got, u)
