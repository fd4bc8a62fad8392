"""Two-level (leapfrog) step loops: neptune_hip_step_loop_leapfrog over a lowered apply's __geom entry (three rotating fields,
one launch per step) and its __geomL2 pair entry (four fields, two steps per pass over HBM, both states stored:
csrc/kernels/apply_march2.hpp).  The bar is bit-exact, no tolerance: both returned states against the oracle running
@step with the rotation done in numpy."""
import ctypes as C

import numpy as np
import pytest

import helpers
import leapfrog_cases as lc

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 3, 7, 12, 37]          # 37: 18 single launches / 8 pair launches are replayed as a graph, twice


@pytest.fixture(scope="module")
def nh():
    import torch
    from neptune_hip import _capi, apply, fields, lowering

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering = torch, _capi, apply, fields, lowering
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    return ns


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return tmp_path_factory.mktemp("leapfrog_modules")


@pytest.fixture(autouse=True)
def pairs_forced_on(monkeypatch, cache):
    """the loop takes pairs only for fields of >= 4e6 cells and only where they measure faster; the parity cases here are
    small, so lift the threshold and switch the measurement off (then: the largest grouping offered)"""
    monkeypatch.setenv("NEPTUNE_HIP_CHAIN_MIN_CELLS", "0")
    monkeypatch.setenv("NEPTUNE_HIP_TUNE", "0")
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(cache))


class Case:
    """one module and its initial data.  Windows: 32 kept rows of 36 (3 x 12 waves; 28 of 32 with a coefficient field, 16 of 24
    at radius 2: two stages lose two rows per side each), 120 kept fp64 / 240 fp32 columns per wave span: every shape below has window seams along J and K, and
    `chunk` planes / rows per chunk put chunk seams inside the field."""

    def __init__(self, shape, elem="f64", radius=1, coef=False, origin=None, bounds=None, chunk=5):
        self.shape, self.elem, self.radius, self.coef, self.chunk = tuple(shape), elem, radius, coef, chunk
        self.origin = list(origin) if origin is not None else [0] * len(shape)
        rel = bounds if bounds is not None else ([radius] * len(shape), [n - radius for n in shape])
        self.bounds = ([o + b for o, b in zip(self.origin, rel[0])], [o + b for o, b in zip(self.origin, rel[1])])
        self.text = lc.module_text(shape, elem=elem, radius=radius, coef=coef, origin=origin, bounds=bounds)
        self.dtype = np.float64 if elem == "f64" else np.float32

    def data(self):
        u0 = helpers.hash_field(self.shape, self.dtype, seed=31)
        um1 = helpers.hash_field(self.shape, self.dtype, seed=32)
        extra = [(0.5 + 0.25 * helpers.hash_field(self.shape, self.dtype, seed=33)).astype(self.dtype)] if self.coef else []
        return u0, um1, extra

    def oracle(self, steps):
        """-> (u(steps), u(steps - 1))"""
        m = helpers.oracle.Module.parse(self.text)
        cur, prev, extra = self.data()
        cur, prev = cur.copy(), prev.copy()
        nxt = np.zeros_like(cur)
        for _ in range(steps):
            m.call("step", nxt, cur, prev, *extra)
            prev, cur, nxt = cur, nxt, prev
        return cur, prev


CASES = {
    "r3_f64": Case((12, 50, 256)),
    "r3_f64_coef": Case((12, 50, 256), coef=True),
    "r3_f32": Case((12, 50, 528), elem="f32"),
    "r3_f64_radius2": Case((14, 50, 256), radius=2),
    "r3_f64_shifted_origin": Case((12, 50, 256), origin=[5, -3, 7]),
    "r3_f64_tight_bounds_coef": Case((16, 50, 256), coef=True, bounds=([2, 3, 9], [13, 44, 201])),   # copy-through bands inside
    "r2_f64": Case((70, 256), chunk=16),
    "r2_f32_coef": Case((70, 528), elem="f32", coef=True, chunk=16),
    "r2_f64_radius2_coef_shifted": Case((70, 256), radius=2, coef=True, origin=[-4, 11], bounds=([3, 5], [66, 250]), chunk=16),
}


def compiled(nh, case):
    mod = nh.lowering.compile_module(case.text)
    return mod, mod.geom_entry("wave")


def device_fields(nh, case, nfields):
    """fields[0] = u(0), fields[1] = u(-1), NaN-filled scratch fields, the extra inputs"""
    u0, um1, extra = case.data()
    fs = [nh.fields.DeviceField.from_numpy(u0, case.origin), nh.fields.DeviceField.from_numpy(um1, case.origin)]
    for _ in range(nfields - 2):
        f = nh.fields.DeviceField.empty_like(fs[0])
        f.tensor.fill_(float("nan"))
        fs.append(f)
    ex = [nh.fields.DeviceField.from_numpy(e, case.origin) for e in extra]
    return fs, ex


def run_loop(nh, case, entry, nfields, steps, cfg="short chunks"):
    """-> (u(steps), u(steps - 1), single launches, pair launches)"""
    fs, ex = device_fields(nh, case, nfields)
    geom = nh.apply.geom_for([fs[0], fs[1]] + ex, fs[2], case.bounds)
    if cfg == "short chunks":
        cfg = nh.apply.make_cfg(chunk=case.chunk)
    cur, prev = nh.apply.step_loop_leapfrog(entry, geom, fs, ex, steps=steps, cfg=cfg)
    nh.torch.cuda.synchronize()
    singles, pairs = nh.apply.leapfrog_launch_counts()
    assert sorted({cur, prev}) == sorted([cur, prev]) and 0 <= cur < nfields and 0 <= prev < nfields and cur != prev
    return fs[cur].numpy().copy(), fs[prev].numpy().copy(), singles, pairs


def check_states(got_cur, got_prev, want_cur, want_prev, what):
    assert helpers.bits_equal(got_cur, want_cur), f"{what}: u(steps)\n" + helpers.mismatch_report(got_cur, want_cur)
    assert helpers.bits_equal(got_prev, want_prev), f"{what}: u(steps - 1)\n" + helpers.mismatch_report(got_prev, want_prev)


@pytest.mark.parametrize("name", ["r3_f64", "r2_f64"])
def test_every_step_count_on_three_and_on_four_fields(nh, name):
    """three fields: single launches only, period 3; four fields: pairs (asserted through the loop's launch counters), an odd
    count ends with one single launch.  Both states against the oracle, every step count."""
    case = CASES[name]
    mod, entry = compiled(nh, case)
    assert entry.fn_leapfrog2 is not None
    for steps in STEPS:
        want_cur, want_prev = case.oracle(steps)
        c3, p3, singles, pairs = run_loop(nh, case, entry, 3, steps)
        assert (singles, pairs) == (steps, 0)
        check_states(c3, p3, want_cur, want_prev, f"{name}, three fields, {steps} steps")
        c4, p4, singles, pairs = run_loop(nh, case, entry, 4, steps)
        assert (singles, pairs) == (steps % 2, steps // 2), "pair launches did not run although forced on"
        check_states(c4, p4, want_cur, want_prev, f"{name}, four fields, {steps} steps")


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("r3_f64", "r2_f64")])
def test_element_types_radii_coefficient_fields_origins_and_bounds(nh, name):
    case = CASES[name]
    mod, entry = compiled(nh, case)
    assert entry.fn_leapfrog2 is not None
    for steps in (2, 7, 37):
        want_cur, want_prev = case.oracle(steps)
        c4, p4, singles, pairs = run_loop(nh, case, entry, 4, steps)
        assert (singles, pairs) == (steps % 2, steps // 2)
        check_states(c4, p4, want_cur, want_prev, f"{name}, pairs, {steps} steps")
    want_cur, want_prev = case.oracle(7)
    c3, p3, singles, pairs = run_loop(nh, case, entry, 3, 7)
    assert (singles, pairs) == (7, 0)
    check_states(c3, p3, want_cur, want_prev, f"{name}, singles, 7 steps")
    # whole-field chunks as well (the launch's own choice)
    c4, p4, _, pairs = run_loop(nh, case, entry, 4, 7, cfg=None)
    assert pairs == 3
    check_states(c4, p4, want_cur, want_prev, f"{name}, pairs, automatic chunks")


@pytest.mark.parametrize("name", ["r3_f64_coef", "r3_f64_radius2", "r2_f64_radius2_coef_shifted"])
def test_one_pair_launch_equals_two_single_launches(nh, name):
    case = CASES[name]
    mod, entry = compiled(nh, case)
    fs, ex = device_fields(nh, case, 4)
    geom = nh.apply.geom_for([fs[0], fs[1]] + ex, fs[2], case.bounds)
    st = nh.fields.current_stream_ptr()
    for chunk in (0, case.chunk):
        cfg = nh.apply.make_cfg(chunk=chunk)
        v1, w1 = nh.fields.DeviceField.empty_like(fs[0]), nh.fields.DeviceField.empty_like(fs[0])
        ins = (C.c_void_p * (2 + len(ex)))(fs[0].ptr, fs[1].ptr, *[e.ptr for e in ex])
        assert entry.fn(C.byref(geom), ins, v1.ptr, st, None) == 0
        ins2 = (C.c_void_p * (2 + len(ex)))(v1.ptr, fs[0].ptr, *[e.ptr for e in ex])
        assert entry.fn(C.byref(geom), ins2, w1.ptr, st, None) == 0
        for f in (fs[2], fs[3]):
            f.tensor.fill_(float("nan"))
        assert entry.fn_leapfrog2(C.byref(geom), ins, fs[2].ptr, fs[3].ptr, st, C.byref(cfg)) == 0
        nh.torch.cuda.synchronize()
        assert helpers.bits_equal(fs[2].numpy(), v1.numpy()), f"v, chunk {chunk}\n" + helpers.mismatch_report(fs[2].numpy(), v1.numpy())
        assert helpers.bits_equal(fs[3].numpy(), w1.numpy()), f"w, chunk {chunk}\n" + helpers.mismatch_report(fs[3].numpy(), w1.numpy())
    want_cur, want_prev = case.oracle(2)
    check_states(fs[3].numpy(), fs[2].numpy(), want_cur, want_prev, name)


def test_geometries_and_buffers_the_pair_entry_cannot_take(nh):
    """ragged rows and an output in the previous state's buffer: NEPTUNE_HIP_EUNSUPPORTED, nothing launched; the loop then
    runs single launches and computes the same bits"""
    ragged = Case((10, 20, 100))                    # rows of 800 bytes: not whole 64-byte granules
    mod, entry = compiled(nh, ragged)
    fs, ex = device_fields(nh, ragged, 4)
    geom = nh.apply.geom_for(fs[:2], fs[2], ragged.bounds)
    st = nh.fields.current_stream_ptr()
    ins = (C.c_void_p * 2)(fs[0].ptr, fs[1].ptr)
    for f in (fs[2], fs[3]):
        f.tensor.fill_(7.0)
    assert entry.fn_leapfrog2(C.byref(geom), ins, fs[2].ptr, fs[3].ptr, st, None) == nh.capi.EUNSUPPORTED
    nh.torch.cuda.synchronize()
    assert bool((fs[2].tensor == 7.0).all()) and bool((fs[3].tensor == 7.0).all())
    for steps in (3, 12):
        want_cur, want_prev = ragged.oracle(steps)
        c4, p4, singles, pairs = run_loop(nh, ragged, entry, 4, steps, cfg=None)
        assert (singles, pairs) == (steps, 0)
        check_states(c4, p4, want_cur, want_prev, f"ragged rows, {steps} steps")

    case = CASES["r3_f64"]
    mod, entry = compiled(nh, case)
    fs, ex = device_fields(nh, case, 4)
    geom = nh.apply.geom_for(fs[:2], fs[2], case.bounds)
    ins = (C.c_void_p * 2)(fs[0].ptr, fs[1].ptr)
    before = [f.numpy().copy() for f in fs[:3]]
    fs[2].tensor.fill_(7.0)
    for out_v, out_w in ((fs[2], fs[1]), (fs[1], fs[2]), (fs[2], fs[0]), (fs[2], fs[2])):   # w into p's buffer, v into p's, w into u's, v == w
        assert entry.fn_leapfrog2(C.byref(geom), ins, out_v.ptr, out_w.ptr, st, None) == nh.capi.EUNSUPPORTED
    nh.torch.cuda.synchronize()
    assert helpers.bits_equal(fs[0].numpy(), before[0]) and helpers.bits_equal(fs[1].numpy(), before[1])
    assert bool((fs[2].tensor == 7.0).all())
    # a launch region restricted along dim 1 is not the chain kernel's either
    region = ([0, 4, 0], list(case.shape))
    g2 = nh.apply.geom_for(fs[:2], fs[2], case.bounds, region)
    assert entry.fn_leapfrog2(C.byref(g2), ins, fs[2].ptr, fs[3].ptr, st, None) == nh.capi.EUNSUPPORTED


def test_graph_replayed_and_plain_launches_agree(nh):
    """37 steps in one call (graphs replayed) == 37 calls of one step each, carried over through the returned indices
    == the same with NEPTUNE_HIP_NO_PAIRS"""
    case = CASES["r3_f64_coef"]
    mod, entry = compiled(nh, case)
    loop_cur, loop_prev, _, pairs = run_loop(nh, case, entry, 4, 37)
    assert pairs == 18
    fs, ex = device_fields(nh, case, 4)
    geom = nh.apply.geom_for([fs[0], fs[1]] + ex, fs[2], case.bounds)
    order = list(range(4))             # one step per call: fields reordered so that (cur, prev) come first again
    for _ in range(37):
        view = [fs[i] for i in order]
        cur, prev = nh.apply.step_loop_leapfrog(entry, geom, view, ex, steps=1, cfg=nh.apply.make_cfg(chunk=case.chunk))
        rest = [i for k, i in enumerate(order) if k not in (cur, prev)]
        order = [order[cur], order[prev]] + rest
    nh.torch.cuda.synchronize()
    check_states(fs[order[0]].numpy(), fs[order[1]].numpy(), loop_cur, loop_prev, "one call of 37 steps against 37 calls")


def test_no_pairs_switch_and_size_threshold(nh, monkeypatch):
    case = CASES["r3_f64"]
    mod, entry = compiled(nh, case)
    want_cur, want_prev = case.oracle(12)
    monkeypatch.setenv("NEPTUNE_HIP_NO_PAIRS", "1")
    c, p, singles, pairs = run_loop(nh, case, entry, 4, 12)
    assert (singles, pairs) == (12, 0)
    check_states(c, p, want_cur, want_prev, "NEPTUNE_HIP_NO_PAIRS")
    monkeypatch.delenv("NEPTUNE_HIP_NO_PAIRS")
    monkeypatch.delenv("NEPTUNE_HIP_CHAIN_MIN_CELLS")          # 150k cells: below the default threshold
    c, p, singles, pairs = run_loop(nh, case, entry, 4, 12)
    assert (singles, pairs) == (12, 0)
    check_states(c, p, want_cur, want_prev, "default size threshold")
    monkeypatch.setenv("NEPTUNE_HIP_CHAIN_MIN_CELLS", "0")
    monkeypatch.delenv("NEPTUNE_HIP_TUNE")                     # measured choice: either grouping, the same bits
    c, p, singles, pairs = run_loop(nh, case, entry, 4, 12)
    assert (singles, pairs) in ((12, 0), (0, 6))
    check_states(c, p, want_cur, want_prev, "measured choice")


def test_torch_tensors_and_a_radius_4_step_without_a_pair_entry(nh):
    """an apply that does not qualify for pairs (here: input 1 read at an offset) still gets the rotating loop and graph replay;
    plain torch tensors are accepted as fields"""
    shape = (10, 20, 128)
    text = lc.module_text(shape, prev_offset=[0, 0, 1])
    mod = nh.lowering.compile_module(text)
    entry = mod.geom_entry("wave")
    assert entry.fn_leapfrog2 is None
    u0 = helpers.hash_field(shape, np.float64, seed=31)
    um1 = helpers.hash_field(shape, np.float64, seed=32)
    ts = [nh.torch.from_numpy(u0).cuda(), nh.torch.from_numpy(um1).cuda(), nh.torch.zeros(shape, dtype=nh.torch.float64, device="cuda"),
          nh.torch.zeros(shape, dtype=nh.torch.float64, device="cuda")]
    fa = nh.fields.DeviceField((0, 0, 0), shape, nh.capi.F64, ts[0])
    geom = nh.apply.geom_for([fa, fa], fa, ([1, 1, 1], [n - 1 for n in shape]))
    cur, prev = nh.apply.step_loop_leapfrog(entry, geom, ts, steps=40)
    nh.torch.cuda.synchronize()
    assert nh.apply.leapfrog_launch_counts() == (40, 0)
    m = helpers.oracle.Module.parse(text)
    c, p, n = u0.copy(), um1.copy(), np.zeros(shape)
    for _ in range(40):
        m.call("step", n, c, p)
        p, c, n = c, n, p
    check_states(ts[cur].cpu().numpy(), ts[prev].cpu().numpy(), c, p, "no pair entry, 40 steps")
