"""The slab fuzz cases (tests/slab_fuzz_cases.py) without a GPU: every seed generates the same text twice, verifies and
lowers to the applies its meta describes; nothing in it is something the slab runtime refuses (a refusal is abort() in the
calling process, so the GPU test must never meet one); the seed list times its decompositions covers what the generator is
for -- asserted, not described; one seed per rank cross-compiles for gfx950."""
import numpy as np
import pytest

import slab_fuzz_cases as sfc
import helpers
from helpers import oracle

from neptune_hip import lowering

SEEDS = sfc.SEEDS
COMPILE_SEEDS = [21, 65, 6, 8]        # one per rank


@pytest.fixture(scope="module")
def cases():
    out = {}
    for seed in SEEDS:
        text, meta = sfc.gen_slab_module(seed)
        out[seed] = (text, meta, sfc.decompositions(meta, seed), lowering.to_hip(text))
    return out


def test_the_seed_list_is_within_its_budget(cases):
    """a cap that keeps the fuzz from hiding gaps: every seed runs on the GPU (the GPU file parametrises over this very list
    and skips none), few enough of them that each stays a test of a few seconds"""
    assert len(SEEDS) <= 16 and len(set(SEEDS)) == len(SEEDS)
    assert sum(1 for s in SEEDS if cases[s][1]["rank"] >= 3) <= 5
    assert set(COMPILE_SEEDS) <= set(SEEDS) and sorted(cases[s][1]["rank"] for s in COMPILE_SEEDS) == [1, 2, 3, 4]
    assert set(sfc.GEOM_SEEDS) <= set(SEEDS) and 6 <= len(sfc.GEOM_SEEDS) <= 10
    import test_slab_fuzz_gpu as gpu
    assert gpu.SEEDS == SEEDS
    src = (helpers.REPO / "tests" / "test_slab_fuzz_gpu.py").read_text()
    assert "pytest.skip" not in src and "mark.skip" not in src and "xfail" not in src


@pytest.mark.parametrize("seed", SEEDS)
def test_seed_lowers_to_what_its_meta_describes(cases, seed):
    text, meta, decs, (src, report) = cases[seed]
    text2, meta2 = sfc.gen_slab_module(seed)
    assert text2 == text and meta2 == meta                               # deterministic
    assert [[(s.start, s.stop, s.radius) for s in d] for d in sfc.decompositions(meta, seed)] == \
           [[(s.start, s.stop, s.radius) for s in d] for d in decs]
    lowering.verify(text)
    rank, elem = meta["rank"], meta["elem"]
    assert (rank, elem, meta["form"]) == sfc.seed_rank_elem(seed)
    assert len(meta["shape"]) == len(meta["origin"]) == rank
    # shapes: the smallest that still matter
    if rank == 1:
        assert 2000 <= meta["shape"][0] < 5000
    else:
        assert 8 <= meta["shape"][0] <= 40 and all(5 <= n <= 12 for n in meta["shape"][1:-1])
    for fn in ("entry", "staged", "total"):
        applies = [a for a in report["applies"] if a["function"] == fn]
        assert [a["halo0"] for a in applies] == meta["applies"][fn], f"seed {seed} @{fn}"
        assert all(a["rank"] == rank and a["elem"] == (elem if a["kernel"] != "reduce" else "") for a in applies)
        assert max([a["halo0"] for a in applies], default=0) == meta["halo0"][fn]
    sig = {s["name"]: s for s in report["signatures"]}
    for fn in ("entry", "staged", "total"):
        assert len(sig[fn]["args"]) == meta["outs"][fn] + meta["nin"][fn]
    assert sig["total"]["result"]["kind"] == "scalar" and sig["total"]["result"].get("scalar") != "derived"
    # the group is one off-slab (and its members are reported as such); under a slab view run_apply_group runs them in turn
    assert len(report["groups"]) == (1 if meta["group"] else 0), f"seed {seed}: group"
    assert src.count("nl::run_apply_group<") == (1 if meta["group"] else 0)
    # the two routes of @total
    fused = "nl::run_apply_reduce_sum<" in src
    assert fused == (meta["total_form"] == "fused") and ("nl::run_reduce_sum(" in src) == (not fused)
    # the two rank-4 forms
    if rank == 4:
        assert ("nl::run_apply_nd<" in src) == (meta["form"] == "nd") and "nl::run_apply_batched<" in src
        assert (meta["halo0"]["entry"] > 0) == (meta["form"] == "nd")


@pytest.mark.parametrize("seed", SEEDS)
def test_nothing_the_slab_runtime_refuses(cases, seed):
    """the contract of lowered_runtime.hpp under neptune_hip_set_slab(), over meta, for every decomposition"""
    text, meta, decs, (src, report) = cases[seed]
    g0, n0 = meta["origin"][0], meta["shape"][0]
    glb, gub = meta["origin"], [o + n for o, n in zip(meta["origin"], meta["shape"])]
    for fn, reaches in meta["applies"].items():
        # one apply with a reach along dim 0 per function at most; it is never behind another one (what it reads is an
        # argument or a pointwise result of arguments: whole_local, ghost planes good)
        assert sum(1 for h in reaches if h > 0) <= 1
        first = next((i for i, h in enumerate(reaches) if h > 0), None)
        assert first is None or all(h == 0 for h in reaches[:first])
    for fn in ("entry", "staged", "total"):
        # unconditional (and conditional) accesses stay inside the global box: apply.bounds keep the reach as a margin
        lb, ub = meta["bounds"][fn]
        h = meta["halo0"][fn]
        assert glb[0] + h <= lb[0] <= ub[0] <= gub[0] - h and all(a <= b for a, b in zip(lb, ub))
        assert all(glb[d] <= lb[d] and ub[d] <= gub[d] for d in range(meta["rank"]))
    for box in [meta["reduce"]] + [b for b in meta["store"].values() if b]:
        assert all(glb[d] <= box[0][d] <= box[1][d] <= gub[d] for d in range(meta["rank"]))
    assert text.count("neptune_ir.reduce") == 1 and 'kind = "sum"' in text
    assert text.count("func.return %sum") == 1                                           # the bare reduce
    assert 1 <= len(decs) <= 3
    H = max(meta["halo0"].values())
    for d in decs:
        world, radius = len(d), d[0].radius
        assert 1 <= world <= 5 and H <= radius <= max(H, 1) + 2 and radius >= 1
        assert d[0].start == g0 and d[-1].stop == g0 + n0
        for r, s in enumerate(d):
            assert (s.rank, s.world, s.radius) == (r, world, radius)
            assert s.r_lo == (radius if r > 0 else 0) and s.r_hi == (radius if r < world - 1 else 0)
            assert world == 1 or s.n_own >= radius                                       # the exchange's own contract
            assert r == 0 or s.start == d[r - 1].stop
            assert tuple(s.glb) == tuple(glb) and tuple(s.gub) == tuple(gub)
            assert s.local_lb[0] >= g0 and s.local_ub[0] <= g0 + n0                      # ghosts inside the global box


def _pairs(cases):
    for seed in SEEDS:
        text, meta, decs, (src, report) = cases[seed]
        for d in decs:
            yield meta, d, report


def test_the_seed_list_covers_what_the_generator_is_for(cases):
    metas = [cases[s][1] for s in SEEDS]
    pairs = list(_pairs(cases))

    def some(pred):
        return [1 for meta, d, rep in pairs if pred(meta, d, rep)]

    def any_rank(pred):
        return [1 for meta, d, rep in pairs for s in d if pred(meta, d, s)]
    assert {(m["rank"], m["elem"]) for m in metas} == {(r, e) for r in (1, 2, 3, 4) for e in ("f64", "f32")}
    assert {len(d) for _, d, _ in pairs} == {1, 2, 3, 4, 5}                              # world 1 to 5
    # radius = halo0, halo0 + 1, halo0 + 2 with a real reach along dim 0: the ghost planes are wider than the apply reads
    for extra in (0, 1, 2):
        for fn in ("entry", "staged"):
            assert some(lambda m, d, rep: m["halo0"][fn] > 0 and d[0].radius == m["halo0"][fn] + extra), (fn, extra)
    assert some(lambda m, d, rep: max(m["halo0"].values()) == 0 and d[0].radius == 1)
    for h in (0, 1, 2, 3):
        assert [1 for m in metas if m["halo0"]["entry"] == h], h
    # thin slabs of both kinds, with ghosts on both sides and on one side only, where a stencil reads them
    for fn in ("entry", "staged"):
        assert any_rank(lambda m, d, s: m["halo0"][fn] > 0 and len(d) > 1 and s.n_own == d[0].radius and s.r_lo and s.r_hi), fn
        assert any_rank(lambda m, d, s: m["halo0"][fn] > 0 and len(d) > 1 and s.n_own == d[0].radius and not (s.r_lo and s.r_hi)), fn
        assert any_rank(lambda m, d, s: m["halo0"][fn] > 0 and d[0].radius < s.n_own <= 2 * d[0].radius and s.r_lo and s.r_hi), fn
    # thinner than the pending split's two edge regions (b <= a: wait first), and thick enough for an interior (b > a)
    for fn in ("entry", "staged"):
        h = lambda m: m["halo0"][fn]
        assert any_rank(lambda m, d, s: h(m) > 0 and s.r_lo and s.r_hi and s.n_own <= 2 * h(m)), fn
        assert any_rank(lambda m, d, s: h(m) > 0 and s.r_lo and s.r_hi and s.n_own > 2 * h(m) and d[0].radius > h(m)), fn
    # a non-zero origin along dim 0, both signs, and a body that reads the dim-0 index there
    assert [1 for m in metas if m["origin"][0] > 0] and [1 for m in metas if m["origin"][0] < 0]
    assert [1 for s in SEEDS if cases[s][1]["origin"][0] != 0 and "arith.index_cast %i0" in cases[s][0]]
    # zero-trip ranks: for the apply, for a sub-box store, for the reduce; a reduce box that excludes a whole rank
    for fn in ("entry", "staged"):
        assert any_rank(lambda m, d, s: sfc.trips(m["bounds"][fn]) > 0 and sfc.trips(sfc.clipped(s, m["bounds"][fn])) == 0), fn
        assert any_rank(lambda m, d, s: m["store"][fn] and sfc.trips(m["store"][fn]) > 0 and
                        sfc.trips(sfc.clipped(s, m["store"][fn])) == 0), fn
        # ... and bounds that begin or end inside a MIDDLE rank
        assert any_rank(lambda m, d, s: s.r_lo and s.r_hi and (s.start < m["bounds"][fn][0][0] < s.stop or
                                                                  s.start < m["bounds"][fn][1][0] < s.stop)), fn
    assert any_rank(lambda m, d, s: sfc.trips(m["reduce"]) > 0 and sfc.trips(sfc.clipped(s, m["reduce"])) == 0)
    assert any_rank(lambda m, d, s: s.r_lo and s.r_hi and (s.start < m["reduce"][0][0] < s.stop or s.start < m["reduce"][1][0] < s.stop))
    assert [1 for m in metas if m["store"]["entry"]] and [1 for m in metas if not m["store"]["entry"]]
    # groups, both rank-4 forms, both routes of the reduce, both ends of @staged, star and box, several inputs
    assert len([1 for m in metas if m["group"]]) >= 2 and {m["rank"] for m in metas if m["group"]} == {2, 3}
    assert {m["form"] for m in metas if m["rank"] == 4} == {"batch", "nd"}
    assert {m["total_form"] for m in metas} == {"fused", "plain"}
    assert {m["staged_last"] for m in metas} == {"time_advance", "pointwise"}
    assert {m["box_footprint"]["entry"] for m in metas} == {True, False}
    assert {m["nin"]["entry"] for m in metas} == {1, 2, 3}
    assert [1 for m in metas if m["other_input_reaches_dim0"]]
    # a march-lowered and a direct-lowered stencil with a reach along dim 0
    kernels = {a["kernel"] for _, _, rep in pairs for a in rep["applies"]
               if a["function"] in ("entry", "staged") and a["halo0"] > 0 and a["rank"] <= 3}
    assert {"march", "direct"} <= kernels, kernels
    # rows: vector-aligned, ragged, and shorter than a wave
    last = [m["shape"][-1] for m in metas if m["rank"] > 1]
    assert [n for n in last if n % 4 == 0] and [n for n in last if n % 2 == 1] and [n for n in last if n < 64]
    # part 4: geometry-level entries of rank 2 and 3, f32 among them, several inputs, a reach of 2-3
    geo = [cases[s][1] for s in sfc.GEOM_SEEDS]
    assert {m["rank"] for m in geo} == {2, 3} and {m["elem"] for m in geo} == {"f64", "f32"}
    assert [1 for m in geo if m["halo0"]["entry"] >= 2] and [1 for m in geo if m["nin"]["entry"] > 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_results_are_finite_and_the_reduce_sums_the_terms(cases, seed):
    """what the GPU test compares with: the oracle on the GLOBAL arrays, nothing slab-aware in it"""
    text, meta, decs, _ = cases[seed]
    dt = sfc.np_dtype(meta)
    m = oracle.Module.parse(text)
    ins = sfc.inputs(meta, 3)
    for fn in ("entry", "staged"):
        outs = [np.full(meta["shape"], -7.25, dtype=dt) for _ in range(meta["outs"][fn])]
        m.call(fn, *outs, *[a.copy() for a in ins[:meta["nin"][fn]]])
        assert all(np.isfinite(o).all() for o in outs)
        if meta["store"][fn] is None:
            assert not (outs[0] == dt(-7.25)).all()
    terms = m.call("terms", ins[0].copy())
    lb, ub = meta["reduce"]
    box = terms[tuple(slice(a - o, b - o) for a, b, o in zip(lb, ub, meta["origin"]))]
    total = m.call("total", ins[0].copy())
    n = box.size
    bound = 2.0 * max(n - 1, 0) * float(np.finfo(dt).eps) * float(np.abs(box.astype(np.float64)).sum())
    import math
    assert abs(float(total) - math.fsum(float(v) for v in box.reshape(-1))) <= bound


@pytest.mark.parametrize("seed", COMPILE_SEEDS)
def test_one_seed_per_rank_cross_compiles(cases, seed, tmp_path, monkeypatch):
    text, meta, decs, _ = cases[seed]
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    mod = lowering.compile_module(text)          # hipcc --offload-arch=gfx950; no device needed
    for fn in ("entry", "staged", "total", "terms"):
        assert hasattr(mod.lib, fn)
    if meta["rank"] <= 3 and meta["halo0"]["entry"] > 0:
        assert mod.geom_entry("entry").halo0 == meta["halo0"]["entry"]
