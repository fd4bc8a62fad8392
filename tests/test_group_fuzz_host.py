"""The group fuzz cases (tests/group_fuzz_cases.py) without a GPU: every seed verifies, lowers to exactly one group with the
members, union inputs, copy-through sources, input maps and launch form its meta says (a seed the lowering does not
recognise as a group FAILS); the seed list covers what the generator exists for; the oracle gives the same bits for the
group module and for every member cut out on its own; one seed per rank cross-compiles for gfx950."""
import numpy as np
import pytest

import group_fuzz_cases as gfc
import helpers
from helpers import bits_equal, mismatch_report, oracle

from neptune_hip import lowering

SEEDS = gfc.SEEDS
COMPILE_SEEDS = [6, 25, 14]        # one per rank, each with rows shorter than a wave


@pytest.fixture(scope="module")
def cases():
    return {seed: gfc.gen_group_module(seed) for seed in SEEDS}


def test_the_seed_list_is_within_its_budget(cases):
    assert 16 <= len(SEEDS) <= 24 and len(set(SEEDS)) == len(SEEDS)
    assert sum(1 for s in SEEDS if cases[s][6]["rank"] == 3) <= 8
    assert set(gfc.ALIAS_SEEDS) <= set(SEEDS) and set(COMPILE_SEEDS) <= set(SEEDS)
    assert sorted(cases[s][6]["rank"] for s in COMPILE_SEEDS) == [1, 2, 3]


@pytest.mark.parametrize("seed", SEEDS)
def test_seed_lowers_to_the_group_its_meta_describes(cases, seed):
    text, shape, origin, elem, M, F, meta = cases[seed]
    assert gfc.gen_group_module(seed)[0] == text                        # deterministic
    assert len(shape) == len(origin) == meta["rank"] and meta["members"] == M and meta["fields"] == F
    lowering.verify(text)
    src, report = lowering.to_hip(text)
    assert len(report["groups"]) == 1, f"seed {seed}: not recognised as one group\n{text}"
    grp = report["groups"][0]
    assert grp["function"] == "entry" and grp["members"] == [f"entry_{m}" for m in range(M)]
    assert grp["inputs"] == meta["inputs"] and len(grp["inputs"]) == F
    assert grp["through"] == meta["through"]
    assert grp["kernel"] == meta["kernel"], f"seed {seed} ({meta['class']}, {meta['mode']})"
    assert grp["rank"] == meta["rank"] and grp["elem"] == elem
    assert src.count("nl::run_apply_group<") == 1
    for m, mp in enumerate(meta["maps"]):
        want = f"neptune_hip::GroupMember<Body_entry_{m}, FP_entry_{m}, {len(mp)}, {', '.join(map(str, mp))}>"
        assert want in src, f"seed {seed}: member {m}'s input map"
    # a result with a second reader: that apply is lowered on its own, after the group
    singles = [a for a in report["applies"] if "group" not in a]
    assert len(singles) == meta["stores"].count("twice") and len(report["applies"]) == M + len(singles)
    # what the aliasing test relies on
    for m, k in meta["foreign"]:
        assert k not in meta["member_fields"][m] and any(k in mf for mf in meta["member_fields"])


def test_the_seed_list_covers_what_the_generator_is_for(cases):
    metas = [cases[s][6] for s in SEEDS]

    def some(pred):
        return [mt for mt in metas if pred(mt)]
    assert {(mt["rank"], mt["elem"]) for mt in metas} == {(r, e) for r in (1, 2, 3) for e in ("f64", "f32")}
    assert len({mt["rank"] for mt in some(lambda mt: mt["members"] == 4)}) >= 2
    assert some(lambda mt: mt["fields"] == 4)
    assert some(lambda mt: mt["subset_map"] and mt["non_identity_through"])
    assert some(lambda mt: mt["fixed_input"])
    assert some(lambda mt: mt["star_plus_box"] and mt["kernel"] == "march")
    assert some(lambda mt: mt["mixed_radius"] and mt["kernel"] == "march")
    assert some(lambda mt: mt["centre_and_offsets"])
    assert some(lambda mt: mt["asymmetric"])
    assert some(lambda mt: len(set(mt["uses_index"])) == 2)
    assert some(lambda mt: mt["zero_trip"]) and some(lambda mt: mt["full_box"])
    assert not some(lambda mt: mt["zero_trip"] and mt["class"] != "zero_trip")
    for kind in ("plain", "bounded", "twice"):
        assert some(lambda mt: kind in mt["stores"]), kind
    # a forwarded member and one that gets a temporary in the same launch
    assert some(lambda mt: "plain" in mt["stores"] and len(set(mt["stores"])) > 1 and mt["kernel"] == "march")
    for kernel in ("march", "direct", "members"):
        assert some(lambda mt: mt["kernel"] == kernel), kernel
    assert len(some(lambda mt: mt["kernel"] == "direct")) >= 2
    assert len(some(lambda mt: mt["class"] == "members2")) >= 1 and len(some(lambda mt: mt["class"] == "members3")) >= 1
    # rows: every offset from a whole number of wave rows, and one shorter than a single wave row, for both types
    for elem, vk in (("f64", 2), ("f32", 4)):
        last = [cases[s][1][-1] for s in SEEDS if cases[s][3] == elem]
        assert {n % (64 * vk) for n in last} >= {0, 1, 64 * vk - 1}, elem
        assert any(n < 64 * vk - 1 for n in last), elem
    assert some(lambda mt: any(o != 0 for o in cases[SEEDS[metas.index(mt)]][2]))
    # the aliasing seeds: (b) needs a field that only other members read; all three launch forms, a sub-box store and a
    # second reader among them
    al = [cases[s][6] for s in gfc.ALIAS_SEEDS]
    assert all(mt["foreign"] for mt in al)
    assert {mt["kernel"] for mt in al} == {"march", "direct", "members"}
    assert {k for mt in al for k in mt["stores"]} == {"plain", "bounded", "twice"}


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_reads_the_group_as_its_members_one_by_one(cases, seed):
    """the comparison target of the GPU tests has no group-specific reading of the text: each member's module, run alone,
    leaves the bits the group module leaves in that member's field"""
    text, shape, origin, elem, M, F, meta = cases[seed]
    dt = np.float64 if elem == "f64" else np.float32
    ins = gfc.inputs(seed, shape, elem, F)
    outs = [np.full(shape, -7.0, dtype=dt) for _ in range(M)]
    oracle.Module.parse(text).call("entry", *outs, *[a.copy() for a in ins])
    plain = [np.full(shape, -7.0, dtype=dt) for _ in range(M)]
    oracle.Module.parse(gfc.plain_module(seed)).call("entry", *plain, *[a.copy() for a in ins])
    inside = tuple(slice(l - o, u - o) for l, u, o in zip(meta["lb"], meta["ub"], origin))
    for m in range(M):
        alone = np.full(shape, -7.0, dtype=dt)
        oracle.Module.parse(gfc.member_module(seed, m)).call("entry", alone, *[a.copy() for a in ins])
        assert bits_equal(alone, outs[m]), f"seed {seed} member {m}: " + mismatch_report(alone, outs[m])
        # outside apply.bounds the raw result is the member's OWN unknown; a plain store leaves the raw result
        own = ins[meta["member_fields"][m][0]]
        mask = np.ones(shape, dtype=bool)
        mask[inside] = False
        assert bits_equal(plain[m][mask], own[mask])
        if meta["stores"][m] == "plain":
            assert bits_equal(plain[m], outs[m])
        assert np.isfinite(outs[m][outs[m] != -7.0]).all()
    if meta["zero_trip"]:
        for m in range(M):
            assert bits_equal(plain[m], ins[meta["member_fields"][m][0]])


@pytest.mark.parametrize("seed", COMPILE_SEEDS)
def test_one_seed_per_rank_cross_compiles(cases, seed, tmp_path, monkeypatch):
    text, shape, origin, elem, M, F, meta = cases[seed]
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    mod = lowering.compile_module(text)          # hipcc --offload-arch=gfx950; no device needed
    assert hasattr(mod.lib, "entry") and len(mod.report["groups"]) == 1
    assert hasattr(mod.lib, mod.report["groups"][0]["geom_symbol"])
