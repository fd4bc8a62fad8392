"""The chain fuzz cases (tests/chain_fuzz_cases.py) without a GPU: what the seed list covers is binding (a seed taken out
of SEEDS so that an item goes missing fails here), every ordinary geometry passes the Python restatement of the chain
kernels' eligibility and every refused one fails it, every module verifies and lowers to the chain entries its meta
names, and the oracle's notion of a launch region -- the planes [a, b) of the chained result, the destination's sentinel
elsewhere -- is pinned against the oracle run plane by plane on the slab of planes that plane depends on."""
import numpy as np
import pytest

import chain_fuzz_cases as cf
import helpers
from helpers import bits_equal, mismatch_report, oracle

from neptune_hip import lowering

SEEDS = cf.SEEDS
ORDINARY = [s for s in SEEDS if cf.seed_class(s) != "refused"]
REFUSED = [s for s in SEEDS if cf.seed_class(s) == "refused"]
COMPILE_SEEDS = [1, 2003]          # a chain (two coefficient fields) and a leapfrog module of rank 2 (the quick compiles)


@pytest.fixture(scope="module")
def metas():
    return {seed: cf.gen_chain_case(seed)[1] for seed in SEEDS}


def coverage(metas):
    """the set of coverage items the metas reach; REQUIRED lists what SEEDS must reach"""
    got = set()
    for seed, mt in metas.items():
        if cf.seed_class(seed) == "refused":
            for g in mt["geometries"]:
                got.add(("refused", g["refused"]))
            continue
        form, rank, elem, radii = mt["form"], mt["rank"], mt["elem"], mt["radii"]
        got.add(("triple", form, rank, elem))
        got.add(("radii", radii))
        got.add(("centre_only", mt["centre_only"]))
        if mt["one_sided"]:
            got.add(("one_sided", seed))
        ent = mt["entries"]
        if rank == 2 and mt["wide"] and elem == "f64" and ent.get(3) and ent[3]["MK"] == 8 and ent[3]["KEEPK"] == 112:
            got.add(("three_applies_wide_rank2_f64_MK8",))
        if rank == 3 and mt["wide"] and 3 in ent and ent[3] is None:
            got.add(("three_applies_refused_wide_rank3",))
        if form == "leapfrog":
            assert mt["leapfrog_capable"]
            got.add(("leapfrog_window", rank, ent[2]["window"] if rank == 3 else None))
        if mt["uses_index"]:
            got.add(("index_argument", form))
        if mt["uses_if"]:
            got.add(("scf_if", form))
        for g in mt["geometries"]:
            G = cf.geom_consts(elem, radii, 2)["G"]
            if g["k_seam"]:
                got.add(("k_seam", form, g["k_seam"][1]))
            if g["j_seam"]:
                got.add(("j_seam", form, g["j_seam"][1]))
            if g["shape"][-1] == 2 * G:
                got.add(("least_row", elem))
            if rank == 3 and g["shape"][1] == 8:
                got.add(("eight_rows",))
            if any(e and g["shape"][0] <= e["WARM"] for e in ent.values()):
                got.add(("dim0_within_warm_up", rank))
            if rank == 2:
                got.add(("rank2_rows_mod4", g["shape"][0] % 4))
            got.add(("region", g["region_kind"]))
            if g["region"]:
                n = g["region"][1][0] - g["region"][0][0]
                if g["chunk"] < n and n % g["chunk"]:
                    got.add(("region_with_ragged_chunk", rank))
            got.add(("bounds", g["bounds_kind"]))
            for d in range(rank):
                if g["bounds_kind"] == "tight" and (g["lb"][d] - g["origin"][d] > radii[d] or g["origin"][d] + g["shape"][d] - g["ub"][d] > radii[d]):
                    got.add(("tight_bounds", rank, d))
                if g["bounds_kind"] == "thin" and g["thin_dim"] == d:
                    got.add(("thin_bounds", rank, d))
            if any(g["origin"]):
                got.add(("shifted_origin", form))
            if any(o < 0 for o in g["origin"]):
                got.add(("negative_origin",))
    return got


REQUIRED = (
    [("triple", f, r, e) for f in ("chain", "leapfrog") for r in (2, 3) for e in ("f64", "f32")]
    + [("triple", "euler", r, "f64") for r in (2, 3)]                     # time_advance is f64 only
    + [("radii", p) for p in cf.PATTERNS[3] + cf.PATTERNS[2] if max(p) == 2]
    + [("centre_only", n) for n in (0, 1, 2)]
    + [("three_applies_wide_rank2_f64_MK8",), ("three_applies_refused_wide_rank3",)]
    + [("leapfrog_window", 3, w) for w in ((3, 12), (4, 8), (3, 8))] + [("leapfrog_window", 2, None)]
    + [("index_argument", f) for f in ("chain", "leapfrog")] + [("scf_if", f) for f in ("chain", "leapfrog")]
    + [(axis, f, e) for axis in ("k_seam", "j_seam") for f in ("chain", "euler", "leapfrog") for e in (-1, 0, 1)]
    + [("least_row", "f64"), ("least_row", "f32"), ("eight_rows",), ("dim0_within_warm_up", 2), ("dim0_within_warm_up", 3)]
    + [("rank2_rows_mod4", r) for r in range(4)]
    + [("region", k) for k in ("none", "inside", "one_plane", "above_bounds")]
    + [("region_with_ragged_chunk", 2), ("region_with_ragged_chunk", 3)]
    + [("bounds", k) for k in ("interior", "tight", "thin")]
    + [("tight_bounds", r, d) for r in (2, 3) for d in range(r)]
    + [("shifted_origin", f) for f in ("chain", "euler", "leapfrog")] + [("negative_origin",)]
    + [("refused", w) for w in ("ragged_row", "reach_leaves_box", "region_dim1")]
)


def test_the_seed_list_is_within_its_budget(metas):
    assert len(set(SEEDS)) == len(SEEDS)
    assert len(ORDINARY) <= 24 and sum(1 for s in ORDINARY if metas[s]["rank"] == 3) <= 10
    assert 2 <= len(REFUSED) <= 3 and all(cf.REFUSED_BASE[s] in ORDINARY for s in REFUSED)     # they take no module of their own
    for s in ORDINARY:
        assert 3 <= len(metas[s]["geometries"]) <= 5
        for g in metas[s]["geometries"]:
            assert int(np.prod(g["shape"])) <= cf.CELL_BUDGET
    assert set(cf.LOOP_SEEDS) <= set(ORDINARY) and set(COMPILE_SEEDS) <= set(ORDINARY)
    per_form = {}
    for s in cf.LOOP_SEEDS:
        per_form.setdefault(metas[s]["form"], []).append(s)
    assert {f: len(v) for f, v in per_form.items()} == {"chain": 2, "euler": 2, "leapfrog": 2}


def test_the_seed_list_covers_what_the_generator_is_for(metas):
    got = coverage(metas)
    missing = [item for item in REQUIRED if item not in got]
    assert not missing, missing
    assert len([i for i in got if i[0] == "one_sided"]) >= 2
    # NaN on never-read cells: in a third of the seeds at least, and on centre-only inputs as well
    with_nan = [s for s in ORDINARY if any(any(g["nan_cells"]) for g in metas[s]["geometries"])]
    assert 3 * len(with_nan) >= len(SEEDS)
    assert any(g["nan_cells"][-1] for s in ORDINARY if metas[s]["centre_only"] for g in metas[s]["geometries"])


def test_window_constants_restate_the_header():
    """March2Geom at the values the header's own comments give (120 of 128 fp64 columns; rows: 44 of 48 on the 3 x 16 window)
    and the one configuration whose kept span is 112"""
    assert cf.geom_consts("f64", (1, 1, 1), 2)["KEEPK"] == 120 and cf.geom_consts("f64", (1, 1, 1), 3)["KEEPK"] == 120
    assert cf.geom_consts("f32", (2, 2, 2), 2)["KEEPK"] == 240 and cf.geom_consts("f32", (1, 1), 3)["MK"] == 8
    assert cf.geom_consts("f64", (2, 2), 3)["MK"] == 8 and cf.geom_consts("f64", (2, 2), 3)["KEEPK"] == 112
    assert cf.geom_consts("f64", (2, 2), 2)["MK"] == 4 and cf.geom_consts("f64", (2, 2), 3)["WARM"] == 8
    assert cf.keepj("chain", 3, (1, 1, 1), 1, 2) == 44 and cf.keepj("chain", 3, (1, 1, 1), 1, 3) == 30
    assert cf.keepj("chain", 3, (2, 2, 2), 1, 2) == 16 and cf.keepj("chain", 3, (2, 2, 2), 1, 2, march2_env=1) == 24
    assert cf.keepj("chain", 3, (2, 2, 2), 1, 3) is None
    assert cf.keepj("leapfrog", 3, (1, 1, 1), 2, 2) == 32 and cf.keepj("leapfrog", 3, (1, 1, 1), 3, 2) == 28
    assert cf.keepj("leapfrog", 3, (2, 2, 2), 2, 2) == 16 and cf.keepj("leapfrog", 3, (1, 2, 1), 2, 2) == 16


def test_every_ordinary_geometry_is_eligible_and_every_refused_one_is_not(metas):
    for s in ORDINARY:
        for gi, g in enumerate(metas[s]["geometries"]):
            assert cf.eligible(metas[s], g), f"seed {s} geometry {gi}: {g}"
    for s in REFUSED:
        for g in metas[s]["geometries"]:
            assert not cf.eligible(metas[s], g), f"seed {s}: {g}"
            # ... while the single-launch entry still takes it: the accesses the body makes stay inside the box
            lo = [min(o[d] for o in metas[s]["offsets"]) for d in range(metas[s]["rank"])]
            hi = [max(o[d] for o in metas[s]["offsets"]) for d in range(metas[s]["rank"])]
            for d in range(metas[s]["rank"]):
                assert g["lb"][d] + lo[d] >= g["origin"][d] and g["ub"][d] + hi[d] <= g["origin"][d] + g["shape"][d]


@pytest.mark.parametrize("seed", ORDINARY)
def test_seed_lowers_to_the_chain_entries_its_meta_names(metas, seed):
    text, mt = cf.gen_chain_case(seed)
    assert text == cf.compile_text(seed) and mt == metas[seed]                  # deterministic
    lowering.verify(text)
    src, report = lowering.to_hip(text)
    rank, nin, T = mt["rank"], mt["nin"], {"f64": "double", "f32": "float"}[mt["elem"]]
    if mt["form"] == "euler":
        assert f'extern "C" int step_ta0__geom2(' in src and f'extern "C" int step_ta0__geom3(' in src
        assert f"neptune_hip::launch_apply_thrice<neptune_hip::ops::EulerFused<Body_op_0, double, {rank}>, double, {rank}, 1, FP_op_0>" in src
    else:
        assert f"neptune_hip::launch_apply_twice<Body_op_0, {T}, {rank}, {nin}, FP_op_0>" in src
        assert f"neptune_hip::launch_apply_thrice<Body_op_0, {T}, {rank}, {nin}, FP_op_0>" in src
    # (the emitter offers the pair entry to every apply with a centre-only input 1 its windows hold, chains included)
    assert (f'extern "C" int op_0__geomL2(' in src) == (nin >= 2 and mt["form"] != "euler" and cf.leapfrog_capable(rank, mt["radii"], nin))
    # the geometry's own text differs from the compiled one in the boxes only
    for gi in range(len(mt["geometries"])):
        lowering.verify(cf.geometry_text(seed, gi))


@pytest.mark.parametrize("seed", COMPILE_SEEDS)
def test_two_rank2_seeds_cross_compile(metas, seed, tmp_path, monkeypatch):
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    mod = lowering.compile_module(cf.compile_text(seed))          # hipcc --offload-arch=gfx950; no device needed
    assert hasattr(mod.lib, "op_0__geom2") and hasattr(mod.lib, "op_0__geom3")
    assert hasattr(mod.lib, "op_0__geomL2") and (seed != 2003 or metas[seed]["form"] == "leapfrog")


def plane_by_plane(seed, gi, mt, ns, planes):
    """planes of the ns-fold chained result, each computed on its own: the oracle on the slab of the ns * R0 planes either side
    that the plane depends on (cut at the field's ends), the slab's cut faces taken out of the bounds"""
    c, geoms = cf._draw(seed)
    g = geoms[gi]
    ins, _ = cf.inputs(seed, gi)
    r0, n0, o0 = mt["radii"][0], g["shape"][0], g["origin"][0]
    out = {}
    for i in planes:
        a, b = max(0, i - ns * r0), min(n0, i + ns * r0 + 1)
        lb, ub = list(g["lb"]), list(g["ub"])
        lb[0] = max(lb[0], o0 + a + (r0 if a > 0 else 0))
        ub[0] = min(ub[0], o0 + b - (r0 if b < n0 else 0))
        if ub[0] <= lb[0]:
            lb[0] = ub[0] = o0 + a                     # no in-bounds plane in reach: copies all the way
        m = oracle.Module.parse(cf.module_text(c, [b - a] + g["shape"][1:], [o0 + a] + g["origin"][1:], lb, ub))
        sl = [np.ascontiguousarray(x[a:b]) for x in ins]
        fn = mt["oracle_function"]
        if mt["form"] == "leapfrog":
            cur, prev = sl[0], sl[1]
            for _ in range(ns):
                nxt = np.full_like(cur, cf.SENTINEL)
                m.call(fn, nxt, cur, prev, *sl[2:])
                cur, prev = nxt, cur
        else:
            cur = sl[0]
            for _ in range(ns):
                nxt = np.full_like(cur, cf.SENTINEL)
                m.call(fn, nxt, cur, *sl[1:])
                cur = nxt
        out[i] = cur[i - a]
    return out


@pytest.mark.parametrize("seed", ORDINARY)
def test_oracle_chains_are_finite_and_a_region_is_the_planes_of_the_whole_result(metas, seed):
    mt = metas[seed]
    steps = 3 if mt["form"] != "leapfrog" else 2
    for gi, g in enumerate(mt["geometries"]):
        states = cf.oracle_states(seed, gi, max(steps, 4))
        ins, masks = cf.inputs(seed, gi)
        inside = tuple(slice(l - o, u - o) for l, u, o in zip(g["lb"], g["ub"], g["origin"]))
        for n, st in enumerate(states[1:], 1):
            # kept cells: finite although the never-read cells hold NaN; the never-read cells of input 0 are copied through
            assert np.isfinite(st[inside]).all(), f"seed {seed} geometry {gi}: apply {n} reads a never-read cell (or overflows)"
            assert np.abs(st[inside]).max() < 1e6
            assert mt["form"] == "euler" or bits_equal(st[masks[0]], ins[0][masks[0]])
        assert sum(int(m.sum()) for m in masks) == sum(g["nan_cells"]) or mt["form"] == "euler"
        if mt["form"] != "euler" and g["nan_cells"][0]:
            assert np.isnan(states[2][masks[0]]).all()
        # what the GPU tests expect of a launch over `region`: the region's planes of the chained result, the sentinel elsewhere
        if g["region"] is None:
            continue
        a, b = g["region"][0][0], g["region"][1][0]
        for ns in sorted(k for k, e in mt["entries"].items() if e):
            want = np.full_like(states[ns], cf.SENTINEL)
            want[a:b] = states[ns][a:b]
            alone = plane_by_plane(seed, gi, mt, ns, range(a, b))
            for i in range(g["shape"][0]):
                if a <= i < b:
                    assert bits_equal(want[i], alone[i]), f"seed {seed} geometry {gi} ns {ns} plane {i}: " + mismatch_report(want[i], alone[i])
                else:
                    assert (want[i] == cf.SENTINEL).all()


@pytest.mark.parametrize("seed", cf.LOOP_SEEDS)
def test_the_loop_seeds_stay_finite_for_eighteen_steps(metas, seed):
    states = cf.oracle_states(seed, 0, 18)
    g = metas[seed]["geometries"][0]
    inside = tuple(slice(l - o, u - o) for l, u, o in zip(g["lb"], g["ub"], g["origin"]))
    assert all(np.isfinite(st[inside]).all() and np.abs(st[inside]).max() < 1e6 for st in states)
