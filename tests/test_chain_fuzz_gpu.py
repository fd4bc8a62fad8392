"""The seeded chain cases (tests/chain_fuzz_cases.py) on the GPU, bit for bit: every module's chain entries (<tag>__geom2,
__geom3, __geomL2: csrc/kernels/apply_march2.hpp) on every one of its geometries -- extents around the window seams, dim-0
extents shorter than the warm-up, shifted origins, tight and one-cell-thick bounds, launch regions along dim 0, the launcher's
own chunk and a drawn one -- against the same number of single launches on the device (so that "the chain differs" and "the
apply differs" come apart) and against the oracle.  Every destination starts as a sentinel, so planes outside the region
must keep it; the inputs hold NaN wherever no stage reads arithmetically (chain and leapfrog forms), so a clamped or rim
load that reaches a kept cell shows; no input is written.  Step loops of 5 and 18 steps, the refused geometries, and the
second radius-2 window (NEPTUNE_HIP_MARCH2=1, read once per process: a child process).  tests/test_chain_fuzz_host.py holds
what the seed list covers.  Only IEEE-exact operations: no tolerance anywhere."""
import ctypes as C
import os
import time
import types

import numpy as np
import pytest

import chain_fuzz_cases as cf
import helpers
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

CHAIN_SEEDS = [s for s in cf.SEEDS if cf.seed_class(s) in ("chain", "euler")]
LEAPFROG_SEEDS = [s for s in cf.SEEDS if cf.seed_class(s) == "leapfrog"]
REFUSED_SEEDS = [s for s in cf.SEEDS if cf.seed_class(s) == "refused"]
# the radius-2 table of launch_march2 is the one with a second window in every build: rank 3, chain and Euler forms
WIDE_RANK3_CHAIN_SEEDS = [s for s in CHAIN_SEEDS if cf.decode(s)[1] == 3 and max(cf.decode(s)[3]) > 1]
KEEP_ALIVE = []                    # ctypes thunks handed to a step loop stay allocated: its graph cache is keyed by them


def sid(seed):
    return f"s{seed:04d}"


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    # a cache filled beforehand (same build) saves the compiles; otherwise they run side by side here
    cache = os.environ.get("NEPTUNE_CHAIN_FUZZ_TEST_CACHE") or str(tmp_path_factory.mktemp("neptune_cache_chainfuzz"))
    os.environ["NEPTUNE_CACHE_DIR"] = cache
    from neptune_hip import _capi, apply, fields, lowering

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering, ns.cache = torch, _capi, apply, fields, lowering, cache
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    texts = [cf.compile_text(seed) for seed in cf.SEEDS]
    t0 = time.time()
    helpers.prefetch_modules(texts)
    print(f"\n[chain fuzz] prefetch of {len(set(texts))} modules: {time.time() - t0:.1f} s")
    return ns


@pytest.fixture(autouse=True)
def chains_forced_on(monkeypatch, nh):
    """step loops chain only fields of >= 4e6 cells and, where they measure, only what measures faster: the cases here are
    small, so lift the threshold and switch the measurement off (then: the largest grouping offered)"""
    monkeypatch.setenv("NEPTUNE_HIP_CHAIN_MIN_CELLS", "0")
    monkeypatch.setenv("NEPTUNE_HIP_TUNE", "0")
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", nh.cache)


@pytest.fixture(scope="module")
def refs():
    """per (seed, geometry), computed once and never written: the inputs and the oracle stepped call by call"""
    cache = {}

    def get(seed, gi, steps):
        key = (seed, gi)
        if key not in cache or len(cache[key][1]) <= steps:
            ins, _ = cf.inputs(seed, gi)
            states = cf.oracle_states(seed, gi, steps)
            for a in ins + states:
                a.setflags(write=False)
            cache[key] = (ins, states)
        return cache[key]
    return get


def sentinel_field(nh, like):
    f = nh.fields.DeviceField.empty_like(like)
    f.tensor.fill_(cf.SENTINEL)
    return f


def compiled(nh, seed, meta):
    mod = nh.lowering.compile_module(cf.compile_text(seed))
    return mod.geom_entry(meta["function"])


def geometry_of(nh, meta, g, fins, out, region=True):
    return nh.apply.geom_for(fins, out, (g["lb"], g["ub"]), g["region"] if region else None)


def region_of(want, g):
    """what a launch over the geometry's region leaves in a sentinel-filled destination"""
    if g["region"] is None:
        return want
    a, b = g["region"][0][0], g["region"][1][0]
    out = np.full_like(want, cf.SENTINEL)
    out[a:b] = want[a:b]
    return out


def describe(seed, meta, gi, g):
    return (f"seed {seed} {meta['form']} rank {meta['rank']} {meta['elem']} radii {meta['radii']} one-sided {meta['one_sided']} "
            f"inputs {meta['nin']} geometry {gi} ({g['kind']}): shape {g['shape']} origin {g['origin']} bounds {g['lb']}..{g['ub']} "
            f"region {g['region']} ({g['region_kind']})")


@pytest.mark.parametrize("seed", CHAIN_SEEDS, ids=sid)
def test_chain_and_euler_entries_on_every_geometry(nh, refs, seed):
    text, meta = cf.gen_chain_case(seed)
    entry = compiled(nh, seed, meta)
    assert entry.fn2 is not None and entry.fn3 is not None
    st = nh.fields.current_stream_ptr()
    problems, combos = [], 0
    for gi, g in enumerate(meta["geometries"]):
        what = describe(seed, meta, gi, g)
        ins, states = refs(seed, gi, 3)
        fins = [nh.fields.DeviceField.from_numpy(a.copy(), g["origin"]) for a in ins]
        arr = lambda first: nh.apply._in_array([first] + fins[1:])        # noqa: E731
        # the same number of single launches, whole field
        single, cur = [fins[0]], fins[0]
        for n in (1, 2, 3):
            nxt = sentinel_field(nh, fins[0])
            gw = geometry_of(nh, meta, g, fins, nxt, region=False)
            assert entry.fn(C.byref(gw), arr(cur), nxt.ptr, st, None) == 0, what
            single.append(nxt)
            cur = nxt
        nh.torch.cuda.synchronize()
        single = [f.numpy().copy() for f in single]
        for n in (1, 2, 3):
            if not bits_equal(single[n], states[n]):
                problems.append(f"{what}\n  {n} single launches vs the oracle: " + mismatch_report(single[n], states[n]))
        out = sentinel_field(nh, fins[0])
        gr = geometry_of(nh, meta, g, fins, out)
        for ns, fn in ((2, entry.fn2), (3, entry.fn3)):
            for chunk in (0, g["chunk"]):
                out.tensor.fill_(cf.SENTINEL)
                cfg = nh.apply.make_cfg(chunk=chunk)
                rc = fn(C.byref(gr), arr(fins[0]), out.ptr, st, C.byref(cfg))
                nh.torch.cuda.synchronize()
                got = out.numpy()
                combos += 1
                if meta["entries"][ns] is None:             # rank 3, radius 2: three rings of five planes do not fit
                    assert rc == nh.capi.EUNSUPPORTED, what
                    assert bool((out.tensor == cf.SENTINEL).all()), what
                    continue
                assert rc == 0, f"{what}\n  {ns} applies per pass, chunk {chunk}: the entry returned {rc}"
                for name, ref in (("single launches", single[ns]), ("the oracle", states[ns])):
                    want = region_of(ref, g)
                    if not bits_equal(got, want):
                        problems.append(f"{what}\n  {ns} applies per pass, chunk {chunk} vs {name}: " + mismatch_report(got, want))
        for k, f in enumerate(fins):
            assert bits_equal(f.numpy(), ins[k]), f"{what}: input {k} was written"
    print(f"\n[chain fuzz] seed {seed}: {combos} (geometry, entry, chunk) combinations")
    assert not problems, "\n".join(problems[:12]) + "\n" + text


@pytest.mark.parametrize("seed", LEAPFROG_SEEDS, ids=sid)
def test_leapfrog_pair_entry_on_every_geometry(nh, refs, seed):
    text, meta = cf.gen_chain_case(seed)
    entry = compiled(nh, seed, meta)
    assert entry.fn_leapfrog2 is not None
    st = nh.fields.current_stream_ptr()
    problems, combos = [], 0
    for gi, g in enumerate(meta["geometries"]):
        what = describe(seed, meta, gi, g)
        ins, states = refs(seed, gi, 2)
        fins = [nh.fields.DeviceField.from_numpy(a.copy(), g["origin"]) for a in ins]
        extra = [f.ptr for f in fins[2:]]
        # two single launches, the rotation done by hand: v = B(u, p, c...), w = B(v, u, c...)
        v1, w1 = sentinel_field(nh, fins[0]), sentinel_field(nh, fins[0])
        gw = geometry_of(nh, meta, g, fins, v1, region=False)
        ins_a = (C.c_void_p * meta["nin"])(fins[0].ptr, fins[1].ptr, *extra)
        ins_b = (C.c_void_p * meta["nin"])(v1.ptr, fins[0].ptr, *extra)
        assert entry.fn(C.byref(gw), ins_a, v1.ptr, st, None) == 0, what
        assert entry.fn(C.byref(gw), ins_b, w1.ptr, st, None) == 0, what
        nh.torch.cuda.synchronize()
        single = [None, v1.numpy().copy(), w1.numpy().copy()]
        for n in (1, 2):
            if not bits_equal(single[n], states[n]):
                problems.append(f"{what}\n  {n} single launches vs the oracle: " + mismatch_report(single[n], states[n]))
        out_v, out_w = sentinel_field(nh, fins[0]), sentinel_field(nh, fins[0])        # buffers of their own
        gr = geometry_of(nh, meta, g, fins, out_w)
        for chunk in (0, g["chunk"]):
            out_v.tensor.fill_(cf.SENTINEL)
            out_w.tensor.fill_(cf.SENTINEL)
            cfg = nh.apply.make_cfg(chunk=chunk)
            rc = entry.fn_leapfrog2(C.byref(gr), ins_a, out_v.ptr, out_w.ptr, st, C.byref(cfg))
            nh.torch.cuda.synchronize()
            combos += 1
            assert rc == 0, f"{what}\n  pair entry, chunk {chunk}: returned {rc}"
            for which, got, n in (("v", out_v.numpy(), 1), ("w", out_w.numpy(), 2)):
                for name, ref in (("single launches", single[n]), ("the oracle", states[n])):
                    want = region_of(ref, g)
                    if not bits_equal(got, want):
                        problems.append(f"{what}\n  pair entry, chunk {chunk}, {which} vs {name}: " + mismatch_report(got, want))
        for k, f in enumerate(fins):
            assert bits_equal(f.numpy(), ins[k]), f"{what}: input {k} was written"
    print(f"\n[chain fuzz] seed {seed}: {combos} (geometry, entry, chunk) combinations")
    assert not problems, "\n".join(problems[:12]) + "\n" + text


def counting(nh, fn, counts, key):
    """fn behind a thunk that counts its calls and what they returned (the one-level loop has no launch counters)"""
    proto = C.CFUNCTYPE(C.c_int, C.POINTER(nh.capi.ApplyGeom), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(nh.capi.LaunchCfg))

    def call(g, ins, out, stream, cfg):
        rc = fn(g, ins, out, stream, cfg)
        counts.setdefault((key, rc), 0)
        counts[(key, rc)] += 1
        return rc
    thunk = proto(call)
    KEEP_ALIVE.append(thunk)
    return thunk


@pytest.mark.parametrize("steps", [5, 18])
@pytest.mark.parametrize("seed", [s for s in cf.LOOP_SEEDS if cf.seed_class(s) != "leapfrog"], ids=sid)
def test_step_loops_of_chains_and_euler_steps(nh, refs, seed, steps):
    """neptune_hip_step_loop_chain over the module's entries: triples, then single launches (pairs where the triple entry
    refuses), against the oracle stepped call by call"""
    text, meta = cf.gen_chain_case(seed)
    entry = compiled(nh, seed, meta)
    g = meta["geometries"][0]
    assert g["region"] is None
    ins, states = refs(seed, 0, 18)
    a = nh.fields.DeviceField.from_numpy(ins[0].copy(), g["origin"])
    b = sentinel_field(nh, a)
    others = [nh.fields.DeviceField.from_numpy(x.copy(), g["origin"]) for x in ins[1:]]
    counts = {}
    counted = types.SimpleNamespace(symbol=entry.symbol, fn=counting(nh, entry.fn, counts, 1), fn2=counting(nh, entry.fn2, counts, 2),
                                    fn3=counting(nh, entry.fn3, counts, 3))
    res = nh.apply.step_loop(counted, a, b, (g["lb"], g["ub"]), steps, others=others, cfg=nh.apply.make_cfg(chunk=g["chunk"]))
    nh.torch.cuda.synchronize()
    assert res is (b if steps % 2 else a)
    what = describe(seed, meta, 0, g) + f", {steps} steps"
    assert bits_equal(res.numpy(), states[steps]), what + "\n" + mismatch_report(res.numpy(), states[steps]) + "\n" + text
    for k, f in enumerate(others):
        assert bits_equal(f.numpy(), ins[k + 1]), f"{what}: input {k + 1} was written"
    ok = {k: counts.get((k, 0), 0) for k in (1, 2, 3)}
    if steps >= 8:
        # a loop this long may measure the groupings first and take any of them: the one-level loop reads NEPTUNE_HIP_TUNE once
        # per process, so what an earlier test of the same process left decides (trial launches pass through the thunks too)
        assert ok[1] + 2 * ok[2] + 3 * ok[3] >= steps, (what, counts)
    elif meta["entries"][3] is not None:                                   # the largest grouping offered: triples, then singles
        assert ok == {1: steps % 3, 2: 0, 3: steps // 3}, (what, counts)
    else:                                                                  # the triple entry refuses: pairs, then singles
        pairs = (steps // 2) & ~1
        assert ok == {1: steps - 2 * pairs, 2: pairs, 3: 0} and counts.get((3, nh.capi.EUNSUPPORTED)) == 1, (what, counts)


@pytest.mark.parametrize("steps", [5, 18])
@pytest.mark.parametrize("seed", [s for s in cf.LOOP_SEEDS if cf.seed_class(s) == "leapfrog"], ids=sid)
def test_step_loops_of_leapfrog_pairs(nh, refs, seed, steps):
    text, meta = cf.gen_chain_case(seed)
    entry = compiled(nh, seed, meta)
    g = meta["geometries"][0]
    ins, states = refs(seed, 0, 18)
    fs = [nh.fields.DeviceField.from_numpy(ins[0].copy(), g["origin"]), nh.fields.DeviceField.from_numpy(ins[1].copy(), g["origin"])]
    fs += [sentinel_field(nh, fs[0]), sentinel_field(nh, fs[0])]
    ex = [nh.fields.DeviceField.from_numpy(x.copy(), g["origin"]) for x in ins[2:]]
    geom = nh.apply.geom_for([fs[0], fs[1]] + ex, fs[2], (g["lb"], g["ub"]))
    cur, prev = nh.apply.step_loop_leapfrog(entry, geom, fs, ex, steps=steps, cfg=nh.apply.make_cfg(chunk=g["chunk"]))
    nh.torch.cuda.synchronize()
    assert nh.apply.leapfrog_launch_counts() == (steps % 2, steps // 2), "pair launches did not run although forced on"
    what = describe(seed, meta, 0, g) + f", {steps} steps"
    assert cur != prev and 0 <= cur < 4 and 0 <= prev < 4
    for name, got, want in (("u(steps)", fs[cur].numpy(), states[steps]), ("u(steps - 1)", fs[prev].numpy(), states[steps - 1])):
        assert bits_equal(got, want), f"{what}: {name}\n" + mismatch_report(got, want) + "\n" + text
    for k, f in enumerate(ex):
        assert bits_equal(f.numpy(), ins[k + 2]), f"{what}: input {k + 2} was written"


@pytest.mark.parametrize("seed", REFUSED_SEEDS, ids=sid)
def test_refused_geometries_leave_the_destination_untouched(nh, seed):
    """a row that is not a whole granule, bounds whose symmetric radius leaves the box, a region on dim 1: every chain entry
    returns EUNSUPPORTED and nothing is launched"""
    text, meta = cf.gen_chain_case(seed)
    entry = compiled(nh, seed, meta)
    st = nh.fields.current_stream_ptr()
    for gi, g in enumerate(meta["geometries"]):
        what = describe(seed, meta, gi, g) + f" refused: {g['refused']}"
        ins, _ = cf.inputs(seed, gi, nan=False)
        fins = [nh.fields.DeviceField.from_numpy(a, g["origin"]) for a in ins]
        out, out2 = sentinel_field(nh, fins[0]), sentinel_field(nh, fins[0])
        gr = geometry_of(nh, meta, g, fins, out)
        arr = nh.apply._in_array(fins)
        assert entry.fn2 is not None and entry.fn3 is not None
        assert entry.fn2(C.byref(gr), arr, out.ptr, st, None) == nh.capi.EUNSUPPORTED, what
        assert entry.fn3(C.byref(gr), arr, out.ptr, st, None) == nh.capi.EUNSUPPORTED, what
        if meta["form"] == "leapfrog":
            assert entry.fn_leapfrog2(C.byref(gr), arr, out.ptr, out2.ptr, st, None) == nh.capi.EUNSUPPORTED, what
        nh.torch.cuda.synchronize()
        assert bool((out.tensor == cf.SENTINEL).all()) and bool((out2.tensor == cf.SENTINEL).all()), what
        for k, f in enumerate(fins):
            assert bits_equal(f.numpy(), ins[k]), f"{what}: input {k} was written"


def test_the_other_radius2_window_in_a_child_process(nh):
    """NEPTUNE_HIP_MARCH2=1 takes the 4 x 8 window for rank-3 footprints of radius 2 (launch_march2, the `wide` table); it is
    read once per process, at the first chain launch: the wide rank-3 chain and Euler seeds again in a fresh process"""
    import subprocess
    import sys
    assert len(WIDE_RANK3_CHAIN_SEEDS) >= 3
    env = dict(os.environ, NEPTUNE_HIP_MARCH2="1", NEPTUNE_CHAIN_FUZZ_TEST_CACHE=nh.cache)
    select = "test_chain_and_euler_entries_on_every_geometry and (" + " or ".join(sid(s) for s in WIDE_RANK3_CHAIN_SEEDS) + ")"
    p = subprocess.run([sys.executable, "-m", "pytest", __file__, "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert f"{len(WIDE_RANK3_CHAIN_SEEDS)} passed" in p.stdout, p.stdout[-2000:]
