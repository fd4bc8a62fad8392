"""The group's geometry-level entry and neptune_hip_step_loop_system on the GPU: one apply_group launch equals
the lowered @entry and the oracle; the hipGraph-replayed system loop equals the host loop of @entry calls and the oracle
iterated step by step, on both field sets; the member-by-member forms give the same bits; a fixed input rides along; every
refused call leaves every buffer as it was.  Only IEEE-exact operations: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import group_cases as gc
import helpers
import system_loop_cases as sc
from helpers import bits_equal, mismatch_report
from test_group_gpu import PRODUCTION, SMALL, inner_bounds, radius2_pair

pytestmark = pytest.mark.gpu

ELEMS = sc.ELEMS
RAGGED = {k: s for k, s in SMALL[1::2]}            # swe (37, 515), pair (11, 18, 261): rows no whole number of lane vectors
STEPS = [0, 1, 2, 15, 16, 17, 33, 37, 50]
MAX_STEPS = max(STEPS)
R2_SHAPE = (12, 20, 256)


def all_texts():
    out = [gc.variant(k, RAGGED[k], *inner_bounds(RAGGED[k]), elem=e) for k in RAGGED for e in ELEMS]
    out += [gc.variant(k, sc.LOOP_SMALL[k], elem=e) for k in sc.LOOP_SMALL for e in ELEMS]
    out += [gc.variant(k, s) for k, s in PRODUCTION.items()]
    out += [radius2_pair(R2_SHAPE), sc.fixed_input_variant(sc.LOOP_SMALL["swe"])]
    return out


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = os.environ.get("NEPTUNE_SYSTEM_LOOP_TEST_CACHE") or str(tmp_path_factory.mktemp("neptune_cache_sys"))
    import neptune_hip as nh
    from neptune_hip import apply, lowering  # noqa: F401
    helpers.prefetch_modules(all_texts())
    return lowering, torch, nh


@pytest.fixture
def no_groups_env():
    saved = os.environ.get("NEPTUNE_HIP_NO_GROUPS")
    yield
    if saved is None:
        os.environ.pop("NEPTUNE_HIP_NO_GROUPS", None)
    else:
        os.environ["NEPTUNE_HIP_NO_GROUPS"] = saved


def set_no_groups(on):
    if on:
        os.environ["NEPTUNE_HIP_NO_GROUPS"] = "1"
    else:
        os.environ.pop("NEPTUNE_HIP_NO_GROUPS", None)


def dev(torch, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def same(got, want, what):
    for m, (a, b) in enumerate(zip(got, want)):
        assert bits_equal(a, b), f"{what}, field {m}: " + mismatch_report(a, b)


def host_loop(mod, torch, ins, steps, fixed=()):
    """`steps` swapped @entry calls -> (newest state, the state before it), as numpy arrays"""
    cur, nxt = dev(torch, ins), [t.clone() for t in dev(torch, ins)]
    fx = dev(torch, fixed)
    for _ in range(steps):
        mod.call("entry", *nxt, *cur, *fx)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    return host(cur), host(nxt)


def run_loop(nh, torch, entry, bounds, ins, steps, fixed=(), cfg=None, explicit_stream=False, fill=-3.0):
    """step_loop_system from `ins` -> (set holding the newest state, the other set, the returned list is the right one)"""
    cur = dev(torch, ins)
    nxt = [torch.full_like(t, fill) for t in cur]
    fx = dev(torch, fixed)
    torch.cuda.synchronize()
    if explicit_stream:
        s = torch.cuda.Stream()
        newest = nh.apply.step_loop_system(entry, bounds, cur, nxt, fx, steps, cfg=cfg, stream=s.cuda_stream)
        s.synchronize()
    else:
        newest = nh.apply.step_loop_system(entry, bounds, cur, nxt, fx, steps, cfg=cfg)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(newest, nxt if steps % 2 else cur))
    other = cur if steps % 2 else nxt
    return host(newest), host(other), host(fx)


def interior(shape):
    return [1] * len(shape), [n - 1 for n in shape]


# ---------------------------------------------------------------- 1. one launch of the group entry
@pytest.mark.parametrize("elem", list(ELEMS))
@pytest.mark.parametrize("kind", list(RAGGED))
def test_apply_group_equals_the_lowered_entry_and_the_oracle(env, no_groups_env, kind, elem):
    lowering, torch, nh = env
    dtype, shape = ELEMS[elem], RAGGED[kind]
    lb, ub = inner_bounds(shape)                       # apply.bounds strictly inside the box
    text = gc.variant(kind, shape, lb, ub, elem)
    ins = gc.inputs(kind, shape, dtype)
    want = gc.oracle_run(text, shape, dtype, ins)
    mod = lowering.compile_module(text)
    entry = mod.group_entry("entry")
    n = gc.NOUT[kind]
    d_ins = dev(torch, ins)
    set_no_groups(False)
    called = [torch.full_like(t, -7.0) for t in d_ins]
    mod.call("entry", *called, *d_ins)
    torch.cuda.synchronize()
    same(host(called), want, f"{kind} {elem} @entry vs oracle")
    for no_groups in (False, True):
        set_no_groups(no_groups)
        outs = [torch.full_like(t, -7.0) for t in d_ins]
        before = nh.apply.group_launch_counts()
        nh.apply.apply_group(entry, d_ins, outs, (lb, ub))
        torch.cuda.synchronize()
        after = nh.apply.group_launch_counts()
        assert (after[0] - before[0], after[1] - before[1]) == ((0, n) if no_groups else (1, 0))
        same(host(outs), want, f"{kind} {elem} apply_group (no_groups={no_groups}) vs oracle")
        same(host(outs), host(called), f"{kind} {elem} apply_group (no_groups={no_groups}) vs @entry")
        # a launch region restricted along dim 0: inside it what each member's own entry computes on the same geometry,
        # outside it nothing is written
        r0, r1 = 3, shape[0] - 5
        region = ([r0] + [0] * (len(shape) - 1), [r1] + list(shape[1:]))
        outs = [torch.full_like(t, -7.0) for t in d_ins]
        nh.apply.apply_group(entry, d_ins, outs, (lb, ub), region=region)
        torch.cuda.synchronize()
        for m in range(n):
            member = mod.geom_entry("entry", m)
            alone = nh.fields.DeviceField.from_numpy(np.full(shape, -7.0, dtype))
            m_ins = [nh.apply._as_field(d_ins[k]) for k in sc.MEMBER_INPUTS[kind][m]]
            nh.apply.apply_builtin(member, m_ins, alone, (lb, ub), region=region)
            torch.cuda.synchronize()
            got, ref = outs[m].cpu().numpy(), alone.numpy()
            assert bits_equal(got, ref), f"{kind} {elem} region, member {m}: " + mismatch_report(got, ref)
            assert bits_equal(got[r0:r1], want[m][r0:r1])
            assert (got[:r0] == -7.0).all() and (got[r1:] == -7.0).all()


# ---------------------------------------------------------------- 2. the loop against the host loop and the oracle
@pytest.fixture(scope="module")
def small_runs(env):
    """per (kind, elem): module, entry, inputs, and the oracle's states 0 .. MAX_STEPS"""
    lowering, torch, nh = env
    cache = {}

    def get(kind, elem):
        if (kind, elem) not in cache:
            dtype, shape = ELEMS[elem], sc.LOOP_SMALL[kind]
            text = gc.variant(kind, shape, elem=elem)
            mod = lowering.compile_module(text)
            ins = sc.loop_inputs(kind, shape, dtype)
            cache[(kind, elem)] = (mod, mod.group_entry("entry"), ins, sc.oracle_states(text, ins, MAX_STEPS))
        return cache[(kind, elem)]
    return get


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("elem", list(ELEMS))
@pytest.mark.parametrize("kind", list(sc.LOOP_SMALL))
def test_system_loop_equals_the_host_loop_and_the_oracle(env, small_runs, no_groups_env, kind, elem, steps):
    lowering, torch, nh = env
    set_no_groups(False)
    mod, entry, ins, states = small_runs(kind, elem)
    shape = sc.LOOP_SMALL[kind]
    bounds = interior(shape)
    want_new, want_old = host_loop(mod, torch, ins, steps)
    same(want_new, states[steps], f"{kind} {elem} host loop of {steps} steps vs oracle")
    for explicit in (False, True):
        what = f"{kind} {elem} {steps} steps ({'explicit' if explicit else 'default'} stream)"
        newest, other, _ = run_loop(nh, torch, entry, bounds, ins, steps, explicit_stream=explicit)
        same(newest, want_new, what + ": newest set vs host loop")
        same(newest, states[steps], what + ": newest set vs oracle")
        if steps == 0:
            assert all((a == -3.0).all() for a in other), what + ": steps = 0 wrote something"
            assert nh.apply.system_loop_counts() == (0, 0)
        else:
            same(other, states[steps - 1], what + ": the other set holds state steps - 1")
            # the first launch is a plain one, then whole graphs of 16, then the rest plain
            assert nh.apply.system_loop_counts() == (steps, (steps - 1) // 16)
    if steps == 50:
        assert nh.apply.system_loop_counts() == (50, 3)
        # the same buffers again: the cached graph is found (same key) and replayed
        cur, nxt = dev(torch, ins), [torch.full_like(t, -3.0) for t in dev(torch, ins)]
        first = host(nh.apply.step_loop_system(entry, bounds, cur, nxt, steps=steps))
        assert nh.apply.system_loop_counts() == (50, 3)
        for t, a in zip(cur, ins):
            t.copy_(torch.from_numpy(a))
        for t in nxt:
            t.fill_(-3.0)
        second = host(nh.apply.step_loop_system(entry, bounds, cur, nxt, steps=steps))
        assert nh.apply.system_loop_counts() == (50, 3)
        same(first, want_new, "first of two calls")
        same(second, first, "second of two calls on the same buffers")


# ---------------------------------------------------------------- 3. production sizes
@pytest.mark.parametrize("kind", list(PRODUCTION))
def test_production_size_loop_equals_the_host_loop(env, no_groups_env, kind):
    """33 steps at 8192^2 / 512^3 f64; tests/test_group_gpu.py pins @entry to the oracle at these sizes"""
    lowering, torch, nh = env
    set_no_groups(False)
    shape, steps = PRODUCTION[kind], 33
    mod = lowering.compile_module(gc.variant(kind, shape))
    entry = mod.group_entry("entry")
    ins = sc.loop_inputs(kind, shape, np.float64)
    cur, nxt = dev(torch, ins), [t.clone() for t in dev(torch, ins)]
    for _ in range(steps):
        mod.call("entry", *nxt, *cur)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    a, b = dev(torch, ins), [torch.zeros_like(t) for t in cur]
    del ins
    newest = nh.apply.step_loop_system(entry, interior(shape), a, b, steps=steps)
    torch.cuda.synchronize()
    assert nh.apply.system_loop_counts() == (33, 2) and newest[0] is b[0]
    for m in range(gc.NOUT[kind]):
        assert bool(torch.isfinite(newest[m]).all())
        assert torch.equal(newest[m].view(torch.int64), cur[m].view(torch.int64)), f"{kind}: field {m} differs after {steps} steps"
        # ... and the set the last step read holds state steps - 1
        assert torch.equal(a[m].view(torch.int64), nxt[m].view(torch.int64)), f"{kind}: field {m} of the other set differs"


# ---------------------------------------------------------------- 4. the same bits on the other forms
def test_members_group_no_groups_and_an_explicit_tile_give_the_same_bits(env, small_runs, no_groups_env):
    lowering, torch, nh = env
    from neptune_hip import _capi
    steps = 37
    # (a) a group with no group form (radius-2 pair: the union footprint runs on the plane-in-LDS kernel)
    set_no_groups(False)
    text = radius2_pair(R2_SHAPE)
    mod = lowering.compile_module(text)
    assert mod.report["groups"][0]["kernel"] == "members"
    entry = mod.group_entry("entry")
    ins = gc.inputs("pair", R2_SHAPE, np.float64)
    bounds = ([2, 2, 2], [n - 2 for n in R2_SHAPE])
    states = sc.oracle_states(text, ins, steps)
    assert all(np.isfinite(a).all() for s in states for a in s)
    before = nh.apply.group_launch_counts()
    newest, other, _ = run_loop(nh, torch, entry, bounds, ins, steps)
    after = nh.apply.group_launch_counts()
    assert after[0] == before[0] and after[1] > before[1]          # member launches only
    want_new, _ = host_loop(mod, torch, ins, steps)
    same(newest, want_new, "members group: loop vs host loop")
    same(newest, states[steps], "members group: loop vs oracle")
    same(other, states[steps - 1], "members group: the other set")
    assert nh.apply.system_loop_counts() == (37, 2)
    # (b) NEPTUNE_HIP_NO_GROUPS=1 and (c) an explicit tile, on both fixtures
    for kind in sc.LOOP_SMALL:
        mod, entry, ins, states = small_runs(kind, "f64")
        bounds = interior(sc.LOOP_SMALL[kind])
        set_no_groups(True)
        before = nh.apply.group_launch_counts()
        newest, other, _ = run_loop(nh, torch, entry, bounds, ins, steps)
        assert nh.apply.group_launch_counts()[0] == before[0]
        set_no_groups(False)
        same(newest, states[steps], f"{kind} NEPTUNE_HIP_NO_GROUPS=1: newest set")
        same(other, states[steps - 1], f"{kind} NEPTUNE_HIP_NO_GROUPS=1: the other set")
        cfg = nh.apply.make_cfg(_capi.KERNEL_AUTO, 1, 1)
        newest, other, _ = run_loop(nh, torch, entry, bounds, ins, steps, cfg=cfg)
        last = _capi.LaunchCfg()
        assert _capi.load().neptune_hip_last_launch(C.byref(last)) == 1
        assert last.kernel != _capi.KERNEL_MARCH or last.variant == 1
        same(newest, states[steps], f"{kind} explicit tile: newest set")
        same(other, states[steps - 1], f"{kind} explicit tile: the other set")


# ---------------------------------------------------------------- 5. a fixed input
def test_a_fixed_input_rides_along_unchanged(env, no_groups_env):
    lowering, torch, nh = env
    set_no_groups(False)
    shape, steps = sc.LOOP_SMALL["swe"], 37
    text = sc.fixed_input_variant(shape)
    mod = lowering.compile_module(text)
    entry = mod.group_entry("entry")
    assert entry.num_inputs == 4 and entry.num_outputs == 3 and entry.through == [0, 1, 2]
    ins, fixed = sc.loop_inputs("swe", shape, np.float64), sc.fixed_field(shape, np.float64)
    states = sc.oracle_states(text, ins, steps, [fixed])
    want_new, want_old = host_loop(mod, torch, ins, steps, [fixed])
    newest, other, fx = run_loop(nh, torch, entry, interior(shape), ins, steps, [fixed])
    same(newest, want_new, "fixed input: loop vs host loop")
    same(newest, states[steps], "fixed input: loop vs oracle")
    same(other, states[steps - 1], "fixed input: the other set")
    assert bits_equal(fx[0], fixed)
    assert nh.apply.system_loop_counts() == (37, 2)
    plain = sc.oracle_states(gc.variant("swe", shape), ins, 1)
    assert not bits_equal(states[1][0], plain[1][0])               # the field really enters the step


# ---------------------------------------------------------------- 6. refusals
def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def test_every_refusal_returns_its_code_and_touches_nothing(env, small_runs, no_groups_env):
    lowering, torch, nh = env
    from neptune_hip import _capi
    from neptune_hip.geometry import make_geom
    set_no_groups(False)
    lib = _capi.load()
    shape = sc.LOOP_SMALL["swe"]
    box = ([0, 0], list(shape))
    mod, entry, ins, _ = small_runs("swe", "f64")
    fmod = lowering.compile_module(sc.fixed_input_variant(shape))
    fentry = fmod.group_entry("entry")
    a = dev(torch, ins)
    b = [torch.full_like(t, -3.0) for t in a]
    fixed = dev(torch, [sc.fixed_field(shape, np.float64)])[0]
    big = torch.full((2 * shape[0], shape[1]), -5.0, dtype=torch.float64, device="cuda")   # two overlapping views
    everything = a + b + [fixed, big]
    before = host(everything)
    g3 = make_geom(box, interior(shape), [box] * 3)
    g4 = make_geom(box, interior(shape), [box] * 4)
    st = nh.fields.current_stream_ptr()

    def unchanged(what):
        torch.cuda.synchronize()
        same(host(everything), before, what + ": a buffer changed")

    # ---- the group entry
    def call(geom, ins_, outs_):
        return entry.fn(C.byref(geom) if geom is not None else None, ptrs(ins_) if ins_ is not None else None,
                        ptrs(outs_) if outs_ is not None else None, st, None)
    half = big[shape[0] // 2: shape[0] // 2 + shape[0]]            # overlaps big[:shape[0]] by half its rows
    cases = {
        "null geometry": (None, a, b), "null input array": (g3, None, b), "null output array": (g3, a, None),
        "a null input": (g3, [a[0], None, a[2]], b), "a null result": (g3, a, [b[0], b[1], None]),
        "a result that is an input": (g3, a, [b[0], a[2], b[2]]),
        "a result overlapping an input": (g3, [big[:shape[0]], a[1], a[2]], [b[0], half, b[2]]),
        "two results the same buffer": (g3, a, [b[0], b[1], b[1]]),
        "two results overlapping": (g3, a, [big[:shape[0]], half, b[2]]),
        "four inputs described to a group of three": (g4, a + [fixed], b),
    }
    for what, (geom, ins_, outs_) in cases.items():
        assert call(geom, ins_, outs_) == _capi.EINVAL, what
        unchanged(what)
    whole = make_geom(box, box, [box] * 3)                           # apply.bounds = the box: every member reaches outside
    assert call(whole, a, b) == _capi.EOOB
    unchanged("reach outside the inputs")

    # ---- the loop
    def loop(e, geom, n_out, through, fa, fb, fixed_in, steps=5):
        return lib.neptune_hip_step_loop_system(C.cast(e.fn, C.c_void_p), C.byref(geom), n_out, (C.c_int * len(through))(*through),
                                                ptrs(fa), ptrs(fb), ptrs(fixed_in) if fixed_in is not None else None, steps, st, None)
    none4 = [None] * 4
    loops = {
        "n_out = 1": (entry, g3, 1, [0], a[:1], b[:1], None),
        "n_out = 5": (entry, g3, 5, [0, 1, 2, 0, 1], a + a[:2], b + b[:2], None),
        "through out of range": (entry, g3, 3, [0, 1, 3], a, b, None),
        "through negative": (entry, g3, 3, [0, -1, 2], a, b, None),
        "through repeated": (entry, g3, 3, [0, 1, 1], a, b, None),
        "a buffer in both sets": (entry, g3, 3, [0, 1, 2], a, [b[0], a[1], b[2]], None),
        "a buffer twice in one set": (entry, g3, 3, [0, 1, 2], [a[0], a[0], a[2]], b, None),
        "a null buffer": (entry, g3, 3, [0, 1, 2], a, [b[0], None, b[2]], None),
        "a fixed input missing (no array)": (fentry, g4, 3, [0, 1, 2], a, b, None),
        "a fixed input missing (null slot)": (fentry, g4, 3, [0, 1, 2], a, b, none4),
    }
    for what, args in loops.items():
        assert loop(*args) == _capi.EINVAL, what
        unchanged(what)
    assert loop(entry, g3, 3, [0, 1, 2], a, b, None, steps=-1) == _capi.EINVAL
    unchanged("negative steps")
    assert loop(entry, g3, 3, [0, 1, 2], a, b, None, steps=0) == _capi.OK
    unchanged("steps = 0")
    # ... and the same calls go through once they are well-formed
    assert loop(fentry, g4, 3, [0, 1, 2], a, b, [None, None, None, fixed], steps=2) == _capi.OK
    torch.cuda.synchronize()
    assert not bits_equal(b[0].cpu().numpy(), before[3])
