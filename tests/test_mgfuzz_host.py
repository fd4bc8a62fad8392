"""The multigrid fuzz cases (tests/mgfuzz_cases.py) without a GPU.

The one restatement (tests/mg_restatement.py) IS the features' former own copies: on each feature's fixed problems its run,
its numpy_mgcg and its replay reproduce bit for bit what those copies produced, as tools/record_mg_restatement.py recorded it
from the last commit that had them (tests/golden/mg_restatement.json); every recorded problem is run.
What the seed list covers is binding (a seed taken out of SEEDS so that an item goes missing fails here), the restatement of
every seed stays finite and its conjugate gradients never break down -- a condition on the generator's inputs, so that the
GPU tests compare meaningful numbers --, and all seeds together stay within the budget of module texts."""
import json
import time

import numpy as np
import pytest

import mg_restatement as rst
import mgfuzz_cases as fz
import record_mg_restatement as rec

SEEDS = fz.SEEDS
ORDINARY = [s for s in SEEDS if fz.seed_class(s) != "refused"]
REFUSED = [s for s in SEEDS if fz.seed_class(s) == "refused"]
MODULE_CAP = 48


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_mgfuzz_host.py: {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------- the one restatement is the former copies, bit for bit
@pytest.fixture(scope="module")
def recorded():
    """the golden file; every problem in it is one the two tests below run, with the recorder's schedules"""
    doc = json.loads(rec.GOLDEN.read_text())
    assert sorted(doc["solves"]) == sorted(rec.SOLVES) and sorted(doc["cgs"]) == sorted(rec.CGS)
    assert [tuple(s) for s in doc["schedules"]] == list(rec.SCHEDULES)
    assert (doc["cycles"], doc["iters"], doc["sweeps"], doc["coarse_sweeps"]) == (rec.CYCLES, rec.ITERS, rec.SWEEPS, rec.COARSE_SWEEPS)
    return doc


def _same_record(name, got, want):
    diffs = rec.differences(got, want)
    assert not diffs, f"{name}: " + "; ".join(diffs)


@pytest.mark.parametrize("name", sorted(rec.SOLVES))
def test_the_restatement_reproduces_the_recorded_cycles(name, recorded):
    levels = rec.SOLVES[name][0]()
    x0, b = rec.problem_fields(levels)
    for k, (pre, post, cs, every) in enumerate(rec.SCHEDULES):
        rr0, checks = rst.run(levels, x0, b, rec.CYCLES, pre, post, cs, every)
        _same_record(f"{name}, schedule {k}", rec.solve_record(rr0, checks, levels), recorded["solves"][name][k])


@pytest.mark.parametrize("name", sorted(rec.CGS))
def test_the_restatement_reproduces_the_recorded_replays(name, recorded):
    want = recorded["cgs"][name]
    problem = rec.CGS[name][0]()
    mixed = rst.is_mixed(problem)
    x0, b = rec.problem_fields(problem)
    unhex = float.fromhex
    rz0, trace = unhex(want["rz0_used"]), np.array([[unhex(v) for v in row] for row in want["trace"]])
    # with numpy's own sums the recurrences give the recorded scalars: the r . r sequence of the former numpy_mgcg ...
    st, _, _, _, scalars = rst.replay(problem, x0, b, sweeps=rec.SWEEPS, coarse_sweeps=rec.COARSE_SWEEPS, iters=rec.ITERS)
    assert not any(s[3] for s in scalars)
    assert rec.hexes([st.rz0_used, [list(s[:3]) for s in scalars]]) == [want["rz0_used"], want["trace"]], name
    seq = rst.numpy_mgcg(problem, x0, b, rec.ITERS, rec.SWEEPS, rec.COARSE_SWEEPS)
    assert seq[1:] == [row[2] for row in trace.tolist()] and (want["numpy_rr0"] is None or seq[0] == unhex(want["numpy_rr0"])), name
    # ... and driven by them the replay gives the recorded bits in every field, every level and every checked sum
    st, checks, rr0, rz0_ref, _ = rst.replay(problem, x0, b, rz0, trace, rec.SWEEPS, rec.COARSE_SWEEPS)
    fields = {nm: getattr(st, nm) for nm in (("x", "r", "p", "r32", "z32") if mixed else ("x", "r", "p", "z"))}
    got = rec.cg_record(None, fields, checks, rr0, rz0_ref, rec.levels_of(problem))
    del got["numpy_rr0"]                        # checked above
    _same_record(name, got, {k: want[k] for k in got})


# ---------------------------------------------------------------- what the seed list covers
@pytest.fixture(scope="module")
def cases():
    return {seed: fz.decode(seed) for seed in SEEDS}


def coverage_of(c):
    """the coverage items one decoded case reaches"""
    got = set()
    if c["form"] == "refused":
        return {("refused", c["why"])}
    form, rank, n = c["form"], c["rank"], c["n_levels"]
    got |= {("form", form), ("graph", c["graph"]), ("dtype", np.dtype(c["dtype"]).name), ("offset", c["offset"]),
            ("narrowed", form, any(c["narrowed"])), ("levels", n)}
    if c["both_paths"]:
        got.add(("both_paths", form))
    # what a schedule reaches counts on normal data only: on subnormal data every r . r is 0 against 0.  A graph is captured
    # only when two more cycles or iterations may follow the first, plain one: n >= 3
    if not c["tiny"]:
        got.add(("n", form, c["n"]))
        if c["check_every"] < c["n"]:
            got.add(("several_checks", form))
        if c["n"] >= 3:
            got.add(("plain_path_three_times", form) if not c["graph"] else ("graph_replayed", form))
            if c["both_paths"]:
                got.add(("both_paths_with_a_replayed_graph", form))
            if c["graph"] and any(c["stages"]):
                got.add(("graph_replayed_with_stages", form))
            if c["graph"] and "H" in c["kinds"]:
                got.add(("graph_replayed_over_a_halved_pair", form))
            if c["graph"] and any(c["stages"]) and "H" in c["kinds"]:
                got.add(("graph_replayed_with_stages_and_a_halved_pair",))
            if c["graph"] and any(c["narrowed"]):
                got.add(("graph_replayed_under_a_region",))
    for l in range(n - 1):
        kind, axes = c["kinds"][l], c["transferred"][l]
        got.add(("rank_kind", rank, kind))
        if rank == 3:
            got.add(("rank3_subset", axes, kind))
        if l + 2 < n and c["kinds"][l + 1] != kind:
            got.add(("switch", kind + c["kinds"][l + 1]))
        for d in range(rank):
            if d not in axes and c["m"][l][d] == 1:
                got.add(("kept_extent_1",))
            if d in axes and c["m"][l + 1][d] in (1, 2):
                got.add(("coarse_extent", c["m"][l + 1][d]))
    for d in range(rank):
        chain = tuple(c["m"][l][d] for l in range(n))
        got |= {("chain", chain[:k]) for k in range(2, n + 1)}
    if c["m"][0][-1] > 256:
        got.add(("level0_row_beyond_256",))
    if c["m"][-1][-1] < 64:
        got.add(("coarsest_row_below_64",))
    for l in range(n):
        m = c["m"][l]
        for axis in c["stages"][l]:
            lines = int(np.prod(m)) // m[axis]
            got.add(("stage_along", rank, axis))
            got.add(("stage_kernel_axis", axis + 3 - rank))
            if axis == rank - 1 and lines > 64:
                got.add(("contiguous_stage_over_64_lines",))
            if axis == rank - 1 and lines <= 64:
                got.add(("contiguous_stage_one_group",))
            if m[axis] > 32:
                got.add(("line_over_32_cells",))
            if m[axis] <= 2:
                got.add(("line_of_1_or_2_cells",))
        if c["stages"][l] and l >= 1 and c["kinds"][l - 1] == "H":
            got.add(("stages_below_a_halved_pair",))
        if c["stages"][l] and l + 1 < n and c["kinds"][l] == "H":
            got.add(("stages_above_a_halved_pair",))
    if form == "cg-lines":
        got.add(("k0", len(c["stages"][0])))
        if c["kinds"][0] == "H":
            got.add(("k0_over_a_halved_pair",))
        if rank < 3:
            got.add(("k0_rank_below_3",))
    if form == "mixed":
        if "H" in c["kinds"]:
            got.add(("mixed_halved",))
        if any(len(a) < rank for a in c["transferred"]):
            got.add(("mixed_semi_coarsened",))
        if any(c["stages"][1:]):
            got.add(("mixed_stages_below_level_0",))
    for l in range(n):
        axes = c["stages"][l]
        if len(axes) >= 2 and axes != axes[::-1] and (form != "solve" or (c["post"] and l + 1 < n)):
            got.add(("post_sweep_reverses_distinct_stages", form == "solve"))
    if form == "cg-lines" and len(c["stages"][0]) == 3 and c["stages"][0][1] != c["stages"][0][2]:
        got.add(("k0_3_with_distinct_stages_1_and_2",))
    if c["tiny"]:
        got |= {("subnormal", np.dtype(c["dtype"]).name, k) for k in c["kinds"]}
    if form == "solve":
        got |= {("pre", c["pre"]), ("post", c["post"])}
    else:
        got.add(("sweeps", c["sweeps"]))
    return got


SUBSETS3 = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
FORMS = ("solve", "cg", "cg-lines", "mixed")
REQUIRED = (
    [("form", f) for f in FORMS] + [("graph", g) for g in (False, True)] + [("dtype", t) for t in ("float64", "float32")]
    + [("offset", o) for o in (0, 8)] + [("narrowed", f, v) for f in FORMS for v in (False, True)] + [("levels", n) for n in (2, 3, 4)]
    + [("both_paths", f) for f in FORMS]
    + [(item, f) for f in FORMS for item in ("graph_replayed", "plain_path_three_times", "both_paths_with_a_replayed_graph",
                                             "several_checks", "graph_replayed_with_stages", "graph_replayed_over_a_halved_pair")]
    + [("n", f, n) for f in FORMS for n in (1, 2, 3)]
    + [("graph_replayed_with_stages_and_a_halved_pair",), ("graph_replayed_under_a_region",)]
    + [("rank_kind", r, k) for r in (1, 2, 3) for k in "CH"] + [("rank3_subset", a, k) for a in SUBSETS3 for k in "CH"]
    + [("switch", "CH"), ("switch", "HC"), ("kept_extent_1",), ("coarse_extent", 1), ("coarse_extent", 2)]
    + [("chain", ch) for ch in ((263, 131, 65, 32), (264, 132, 66, 33), (262, 131, 65), (261, 130, 65), (14, 7, 3), (16, 8, 4, 2), (5, 2, 1))]
    + [("level0_row_beyond_256",), ("coarsest_row_below_64",)]
    + [("stage_along", r, a) for r in (1, 2, 3) for a in range(r)] + [("stage_kernel_axis", a) for a in (0, 1, 2)]
    + [("contiguous_stage_over_64_lines",), ("contiguous_stage_one_group",), ("line_over_32_cells",), ("line_of_1_or_2_cells",)]
    + [("stages_below_a_halved_pair",), ("stages_above_a_halved_pair",)]
    + [("k0", k) for k in (1, 2, 3)] + [("k0_over_a_halved_pair",), ("k0_rank_below_3",)]
    + [("mixed_halved",), ("mixed_semi_coarsened",), ("mixed_stages_below_level_0",)]
    + [("pre", v) for v in (0, 1, 2)] + [("post", v) for v in (0, 1, 2)] + [("sweeps", v) for v in (1, 2)]
    + [("post_sweep_reverses_distinct_stages", v) for v in (False, True)] + [("k0_3_with_distinct_stages_1_and_2",)]
    + [("subnormal", t, k) for t in ("float64", "float32") for k in "CH"]
    + [("refused", w) for w in fz.REFUSALS]
)


def test_the_seed_list_is_within_its_budget(cases):
    assert len(set(SEEDS)) == len(SEEDS) and 45 <= len(SEEDS) <= 55
    per_form = {f: sum(1 for c in cases.values() if c["form"] == f) for f in FORMS + ("refused",)}
    assert 18 <= per_form["solve"] <= 22 and 8 <= per_form["cg"] <= 12 and 6 <= per_form["cg-lines"] <= 10, per_form
    assert 6 <= per_form["mixed"] <= 10 and 3 <= per_form["refused"] <= 5, per_form
    narrowed = sum(1 for s in ORDINARY if any(cases[s]["narrowed"]))
    assert len(ORDINARY) // 3 <= narrowed <= 2 * len(ORDINARY) // 3 + 1, narrowed
    assert len(ORDINARY) // 5 <= sum(1 for s in ORDINARY if cases[s]["both_paths"]) <= len(ORDINARY) // 3
    # cycles / iterations spread as decode draws them (a third each): the list is not picked for short runs; few subnormal cases
    per_n = {n: sum(1 for s in ORDINARY if cases[s]["n"] == n) for n in (1, 2, 3)}
    assert all(4 * v >= len(ORDINARY) for v in per_n.values()), per_n
    assert 2 <= sum(1 for s in ORDINARY if cases[s]["tiny"]) <= 4
    for c in cases.values():
        assert all(int(np.prod(shape)) <= 300_000 for shape in c["shapes"])
        assert fz.decode(c["seed"]) == c                                   # deterministic
        if c["form"] == "solve":
            assert c["pre"] + c["post"] >= 1


def test_the_seed_list_covers_what_the_generator_is_for(cases):
    got = set().union(*[coverage_of(c) for c in cases.values()])
    missing = [item for item in REQUIRED if item not in got]
    assert not missing, missing


def test_all_seeds_together_stay_within_the_module_budget(cases):
    texts = {job for c in cases.values() for job in fz.case_modules(c)}
    print(f"{len(texts)} distinct module texts")
    assert len(texts) <= MODULE_CAP
    every = {(fz.module_text(n, l, t), l == 0) for n, (t, ext, _, outer) in fz.TEMPLATES.items() for l in range(len(ext))}
    every |= {(fz.module_text(n, 0, np.float64), True) for n, v in fz.TEMPLATES.items() if v[3]}
    assert texts <= every and len(every) <= MODULE_CAP
    from neptune_hip import lowering
    for text, dot in sorted(every):         # every one verifies and lowers; level 0's export their dot-monitored launch
        _, report = lowering.to_hip(text, dot_entries=dot)
        assert not dot or "dot_symbol" in str(report)


def test_templates_nest_and_draws_respect_them(cases):
    for name, (_, extents, transferred, _) in fz.TEMPLATES.items():
        assert fz._native_kinds(extents, transferred) is not None, name
        for shape, (lb, ub), _ in fz.template_levels(name):
            rims = [(a, n - b) for a, b, n in zip(lb, ub, shape)]
            assert all(1 <= r <= 3 for pair in rims for r in pair) and (len(shape) == 1 or len({r for pair in rims for r in pair}) > 1)
    for c in cases.values():
        for l in range(c["n_levels"]):
            lb, ub = c["bounds"][l]
            assert all(a <= s.start and s.stop <= b and s.stop > s.start for a, b, s in zip(lb, ub, fz.where_of(c, l)))
            region = fz.region_of(c, l)
            assert (region is None) == (not c["narrowed"][l])
            if region:      # bounds x region is Omega
                assert all(max(a, ra) == s.start and min(b, rb) == s.stop for a, b, ra, rb, s in zip(lb, ub, *region, fz.where_of(c, l)))
        if c["form"] == "refused":
            continue
        for l in range(c["n_levels"] - 1):
            for d in range(c["rank"]):
                mf, mc_ = c["m"][l][d], c["m"][l + 1][d]
                want = mc_ if d not in c["transferred"][l] else 2 * mc_ + (c["kinds"][l] == "C")
                assert mf == want, (c["seed"], l, d)


# ---------------------------------------------------------------- the reference stays meaningful
@pytest.mark.parametrize("seed", ORDINARY, ids=[f"s{s:04d}" for s in ORDINARY])
def test_the_restatement_of_a_seed_is_finite_and_cg_does_not_break_down(seed):
    c = fz.decode(seed)
    B = fz.build(c)
    if c["form"] == "solve":
        rr0, checks = fz.reference(B)
        assert all(np.isfinite(v[0]) for v in [rr0] + checks)
        assert np.isfinite(B.levels[0].x).all()
    else:
        st, checks, rr0, rz0_ref, scalars = rst.replay(B.problem, B.x0, B.b, sweeps=c["sweeps"], coarse_sweeps=c["coarse_sweeps"], iters=c["n"])
        assert st.rz0_used > 0 and all(not broken and pq > 0 and rz > 0 and np.isfinite(rr) for pq, rz, rr, broken in scalars), scalars
        for a in (st.x, st.r, st.p):
            assert np.isfinite(a).all()
    for l, L in enumerate(B.levels):
        assert np.isfinite(L.x).all() and np.isfinite(L.b[L.where]).all(), l
        outside = np.ones(L.shape, bool)
        outside[L.where] = False
        if l >= 1:          # a coarse level outside Omega: x zero-filled, b what the work field held
            assert not L.x[outside].any() and np.isnan(L.b[outside]).all()
