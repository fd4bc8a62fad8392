"""Seeded random groups of sibling applies (tests/group_fuzz_cases.py) on the GPU, bit for bit against the oracle: the
lowered @entry on the automatic plan, on every march tile of the rank with chunk seams, on both direct forms and member by
member; the group's geometry-level entry; and destinations that alias an input.  Every result field starts as a sentinel,
so a cell no launch wrote shows up; every setting also pins how many launches the group took.  tests/test_group_fuzz_host.py
holds what the seed list covers.  Only IEEE-exact operations: no tolerance anywhere."""
import os
import time

import numpy as np
import pytest

import group_fuzz_cases as gfc
import helpers
from helpers import bits_equal, mismatch_report, oracle

pytestmark = pytest.mark.gpu

ENV_KEYS = ("NEPTUNE_HIP_KERNEL", "NEPTUNE_HIP_VARIANT", "NEPTUNE_HIP_CHUNK", "NEPTUNE_HIP_NO_GROUPS")
SENTINEL = -7.0
NVAR = {3: 8, 2: 3, 1: 1}


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    # a cache filled beforehand (same build) saves the compiles; otherwise they run side by side here
    os.environ["NEPTUNE_CACHE_DIR"] = os.environ.get("NEPTUNE_GROUP_FUZZ_TEST_CACHE") or str(tmp_path_factory.mktemp("neptune_cache_grpfuzz"))
    import neptune_hip as nh
    from neptune_hip import apply, lowering  # noqa: F401  (nh.apply: the group launch counters)
    t0 = time.time()
    helpers.prefetch_modules([gfc.gen_group_module(seed)[0] for seed in gfc.SEEDS])
    print(f"\n[group fuzz] prefetch of {len(gfc.SEEDS)} modules: {time.time() - t0:.1f} s")
    return lowering, torch, nh


@pytest.fixture(scope="module")
def refs():
    """per seed, computed once and never written: the case, its inputs, the oracle's result fields of @entry (on sentinel-
    filled destinations) and the members' raw results"""
    cache = {}

    def get(seed):
        if seed not in cache:
            case = gfc.gen_group_module(seed)
            text, shape, origin, elem, M, F, meta = case
            dt = np.float64 if elem == "f64" else np.float32
            ins = gfc.inputs(seed, shape, elem, F)
            want = [np.full(shape, SENTINEL, dtype=dt) for _ in range(M)]
            oracle.Module.parse(text).call("entry", *want, *[a.copy() for a in ins])
            raw = [np.full(shape, SENTINEL, dtype=dt) for _ in range(M)]
            oracle.Module.parse(gfc.plain_module(seed)).call("entry", *raw, *[a.copy() for a in ins])
            for a in ins + want + raw:
                a.setflags(write=False)
            cache[seed] = (case, dt, ins, want, raw)
        return cache[seed]
    return get


@pytest.fixture
def launch_env():
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def set_env(setting):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(setting)


def row_fills_a_wave(shape, elem):
    """plan_apply's rule for the automatic plan: a march-class kernel is taken once the whole lane vectors of a row (all but
    the last one of a ragged row) fill one wave; shorter rows run on the direct kernel"""
    vk = 2 if elem == "f64" else 4
    n = shape[-1]
    return (n if n % vk == 0 else n // vk * vk - vk) >= 64 * vk


def expected_launches(meta, setting, shape):
    """(fused launches, member launches) the group takes: one multi-output launch wherever it has a fused form.  A group the
    lowering reports as `members` (its union footprint is planned onto an LDS kernel, which has no group form) has one only
    on the direct kernel, which holds any footprint: when that kernel is forced, or when the rows are too short for a
    march-class kernel and every member is planned onto it as well"""
    M = meta["members"]
    if "NEPTUNE_HIP_NO_GROUPS" in setting:
        return (0, M)
    direct = setting.get("NEPTUNE_HIP_KERNEL", "").startswith("direct") or not row_fills_a_wave(shape, meta["elem"])
    if meta["kernel"] == "members" and not direct:
        return (0, M)
    return (1, 0)


def settings_of(meta):
    out = [{}]
    if meta["kernel"] == "march":
        out += [{"NEPTUNE_HIP_VARIANT": str(v), "NEPTUNE_HIP_CHUNK": c} for v in range(NVAR[meta["rank"]]) for c in ("1", "3")]
    return out + [{"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_KERNEL": "direct-flat"}, {"NEPTUNE_HIP_NO_GROUPS": "1"}]


@pytest.mark.parametrize("seed", gfc.SEEDS)
def test_random_group_matches_the_oracle_on_every_launch_form(env, refs, launch_env, seed):
    lowering, torch, nh = env
    (text, shape, origin, elem, M, F, meta), dt, ins, want, raw = refs(seed)
    mod = lowering.compile_module(text)
    assert len(mod.report["groups"]) == 1 and mod.report["groups"][0]["kernel"] == meta["kernel"]
    d_ins = [torch.from_numpy(a.copy()).cuda() for a in ins]
    problems = []
    for s in settings_of(meta):
        set_env(s)
        d_outs = [torch.full(shape, SENTINEL, dtype=d_ins[0].dtype, device="cuda") for _ in range(M)]
        before = nh.apply.group_launch_counts()
        mod.call("entry", *d_outs, *d_ins)
        torch.cuda.synchronize()
        after = nh.apply.group_launch_counts()
        moved = (after[0] - before[0], after[1] - before[1])
        if moved != expected_launches(meta, s, shape):
            problems.append(f"{s}: group launch counters moved by {moved}, expected {expected_launches(meta, s, shape)}")
        for m in range(M):
            got = d_outs[m].cpu().numpy()
            if not bits_equal(got, want[m]):
                problems.append(f"{s} result {m} (fields {meta['member_fields'][m]}, store {meta['stores'][m]}): " + mismatch_report(got, want[m]))
    for k in range(F):      # no launch wrote an input
        assert bits_equal(d_ins[k].cpu().numpy(), ins[k]), f"seed {seed}: input {k} was written"
    assert not problems, f"seed {seed} {meta['class']} rank {meta['rank']} {elem} shape {shape} origin {origin} mode {meta['mode']} " \
        f"maps {meta['maps']} bounds {meta['lb']}..{meta['ub']}\n" + "\n".join(problems) + "\n" + text


@pytest.mark.parametrize("seed", gfc.SEEDS)
def test_group_geometry_entry_matches_the_lowered_entry_and_the_oracle(env, refs, launch_env, seed):
    lowering, torch, nh = env
    from neptune_hip.fields import DeviceField
    (text, shape, origin, elem, M, F, meta), dt, ins, want, raw = refs(seed)
    mod = lowering.compile_module(text)
    entry = mod.group_entry("entry")
    assert entry.num_inputs == F and entry.num_outputs == M and entry.through == meta["through"]
    set_env({})
    d_ins = [torch.from_numpy(a.copy()).cuda() for a in ins]
    called = [torch.full(shape, SENTINEL, dtype=d_ins[0].dtype, device="cuda") for _ in range(M)]
    mod.call("entry", *called, *d_ins)
    torch.cuda.synchronize()
    called = [t.cpu().numpy() for t in called]
    g_ins = [DeviceField.from_numpy(ins[k].copy(), lb=origin) for k in meta["field_of_input"]]      # the union inputs, in the group's order
    for no_groups in (False, True):
        set_env({"NEPTUNE_HIP_NO_GROUPS": "1"} if no_groups else {})
        g_outs = [DeviceField.from_numpy(np.full(shape, SENTINEL, dtype=dt), lb=origin) for _ in range(M)]
        before = nh.apply.group_launch_counts()
        nh.apply.apply_group(entry, g_ins, g_outs, (meta["lb"], meta["ub"]))
        torch.cuda.synchronize()
        after = nh.apply.group_launch_counts()
        assert (after[0] - before[0], after[1] - before[1]) == expected_launches(meta, {"NEPTUNE_HIP_NO_GROUPS": "1"} if no_groups else {}, shape)
        for m in range(M):
            got = g_outs[m].numpy()
            what = f"seed {seed} apply_group (no_groups={no_groups}) member {m}"
            assert bits_equal(got, raw[m]), what + " vs the oracle: " + mismatch_report(got, raw[m])
            # @entry stores that result: whole (plain), into a sub-box (bounded), or whole and then its second reader's
            # result over the sub-box (twice)
            box = tuple(slice(l - o, u - o) for l, u, o in zip(*meta["store_box"][m], origin))
            if meta["stores"][m] == "plain":
                assert bits_equal(got, called[m]), what + " vs @entry: " + mismatch_report(got, called[m])
            elif meta["stores"][m] == "bounded":
                assert bits_equal(np.ascontiguousarray(got[box]), np.ascontiguousarray(called[m][box])), what + " vs @entry inside its store"
            else:
                outside = np.ones(shape, dtype=bool)
                outside[box] = False
                assert bits_equal(got[outside], called[m][outside]), what + " vs @entry outside its second store"
    for k, f in zip(meta["field_of_input"], g_ins):
        assert bits_equal(f.numpy(), ins[k])


def alias_cases():
    out = []
    for seed in gfc.ALIAS_SEEDS:
        meta = gfc.gen_group_module(seed)[6]
        for m in range(meta["members"]):
            out.append((seed, m, meta["member_fields"][m][0]))                 # (a) in place: its own input 0
            foreign = [k for mm, k in meta["foreign"] if mm == m]
            if foreign:
                out.append((seed, m, foreign[0]))                              # (b) an input only OTHER members read
    return out


@pytest.mark.parametrize("seed,member,field", alias_cases(), ids=[f"{s}-m{m}-in{k}" for s, m, k in alias_cases()])
def test_a_destination_that_aliases_an_input(env, refs, launch_env, seed, member, field):
    """run_apply_group decides forwarding from the actual pointers: the member whose destination is an input gets a
    temporary, its siblings still write straight into their fields, in the same launch"""
    lowering, torch, nh = env
    (text, shape, origin, elem, M, F, meta), dt, ins, _, _ = refs(seed)
    h_ins = [a.copy() for a in ins]
    h_outs = [h_ins[field] if m == member else np.full(shape, SENTINEL, dtype=dt) for m in range(M)]
    oracle.Module.parse(text).call("entry", *h_outs, *h_ins)
    mod = lowering.compile_module(text)
    for s in ({}, {"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_NO_GROUPS": "1"}):
        set_env(s)
        d_ins = [torch.from_numpy(a.copy()).cuda() for a in ins]
        d_outs = [d_ins[field] if m == member else torch.full(shape, SENTINEL, dtype=d_ins[0].dtype, device="cuda") for m in range(M)]
        before = nh.apply.group_launch_counts()
        mod.call("entry", *d_outs, *d_ins)
        torch.cuda.synchronize()
        after = nh.apply.group_launch_counts()
        assert (after[0] - before[0], after[1] - before[1]) == expected_launches(meta, s, shape), s
        for m in range(M):
            got = d_outs[m].cpu().numpy()
            assert bits_equal(got, h_outs[m]), f"seed {seed} member {member} -> input {field}, {s}, result {m}: " + mismatch_report(got, h_outs[m])
        for k in range(F):
            got = d_ins[k].cpu().numpy()
            assert bits_equal(got, h_ins[k]), f"seed {seed} member {member} -> input {field}, {s}, input {k}: " + mismatch_report(got, h_ins[k])
