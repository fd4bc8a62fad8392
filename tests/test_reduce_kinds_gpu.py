"""neptune_ir.reduce kinds max | min | l1 | l2 on the device, plain (neptune_hip.apply.reduce and lowered
modules) and fused with an apply (lowered modules).  Expected values come from NumPy, here and in reduce_kinds_cases.

max and min are exact in any order, so they are compared bit for bit.  l1 and l2 run on the tree of "sum": they are
compared bit for bit with reduce_sum of |f| resp. f*f made by torch (same box, same kernel, same tree), and with a serial
NumPy sum within the bound of the sum, 2 (n - 1) eps sum|t_i|.

What the kernels can get wrong is the value of everything that does not count -- dead unroll slots, the lanes past a row's
end, workgroups with an empty run, cells outside the reduced box: it must be the kind's identity, never 0 and never a
loaded value.  All-negative data under max (all-positive under min) shows a leaked 0, NaN outside the box a leaked load.

The slab refusal (lowered_runtime.hpp refuse_slab_reduce) ends the process, so it is not run here; the report field a
ShardedModule refuses on is checked in test_reduce_kinds_lowering.py."""
import math

import numpy as np
import pytest

import helpers
import reduce_cases as rc
import reduce_kinds_cases as kc

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]
ELEM = {F64: "f64", F32: "f32"}
KINDS = kc.KINDS

# (buffer shape, logical origin, [reduced boxes in array indices; None = the whole buffer])
SHAPES = {
    F64: [((3,), (0,), [None]), ((255,), (0,), [None]), ((257,), (0,), [None]), ((1025,), (0,), [None]),
          ((5, 7), (-2, 3), [None, ((1, 2), (4, 6))]), ((33, 1030), (0, 0), [None, ((0, 0), (33, 1029))]),
          ((9, 6, 70), (0, 0, 0), [None, ((1, 1, 1), (8, 5, 69))])],
}
SHAPES[F32] = SHAPES[F64] + [((4099,), (0,), [None])]
# Beyond the issue's table: the smallest shapes at which a workgroup has NO work at all and writes a pure-identity partial.
# The first pass launches min(units, 2048) workgroups of ceil(units / workgroups) units each, so whole workgroups stay
# empty only above 2048: flat, ceil(nvec / 2048) * 2046 >= nvec just past 2048 * 256 cells; box, 8193 one-chunk rows.
IDLE = {
    F64: [((524290,), (0,), [None]), ((8193, 6), (0, 0), [((0, 1), (8193, 5))])],
    F32: [((524292,), (0,), [None]), ((8193, 6), (0, 0), [((0, 1), (8193, 5))])],
}
RANK4 = ((2, 3, 4, 70), [None, ((0, 0, 0, 0), (2, 3, 4, 70)), ((0, 1, 1, 3), (2, 3, 3, 69)),   # bounded: leading indices 0..1
                         ((0, 1, 2, 3), (2, 3, 2, 69))])                                        # ... and an empty one
BOX2, SUB2 = ((-2, 3), (3, 10)), ((-1, 5), (2, 9))
EMPTY2 = ((0, 5), (0, 9))
BOX3, SUB3 = ((0, 0, 0), (9, 6, 70)), ((1, 1, 1), (8, 5, 69))
PW_SHAPE = {F64: (8, 64), F32: (8, 128)}
INNER = {F64: (((1, 0), (7, 64)), ((2, 2), (6, 62))), F32: (((1, 0), (7, 128)), ((2, 4), (6, 124)))}   # (apply.bounds, reduce box inside)


def _texts():
    t = {}
    for dt in DTYPES:
        e = ELEM[dt]
        t["p2", dt] = kc.plain_kinds_module(e, BOX2, [None, SUB2, EMPTY2])
        t["p3", dt] = kc.plain_kinds_module(e, BOX3, [None, SUB3])
        t["p4", dt] = kc.plain_kinds_module(e, ((0,) * 4, RANK4[0]), [None if b is None else b for b in RANK4[1]])
        t["pw", dt] = kc.pointwise_module(e, PW_SHAPE[dt], "absf", KINDS)
        t["pwempty", dt] = kc.pointwise_module(e, PW_SHAPE[dt], "absf", kc.ALL_KINDS, reduce_box=((3, 8), (3, 16)))
        bounds, red = INNER[dt]
        full = ((0, 0), PW_SHAPE[dt])
        t["id", dt] = kc.fused_kinds_module(e, full, bounds, red, kc._pointwise_body(e, 2, "id"), 2, ("l1", "l2"))
        t["abs", dt] = kc.fused_kinds_module(e, full, bounds, red, kc._pointwise_body(e, 2, "absf"), 2, ("sum",))
        t["sq", dt] = kc.fused_kinds_module(e, full, bounds, red, kc._pointwise_body(e, 2, "sq"), 2, ("sum",))
    t["res", F64] = kc.residual_module("f64")
    t["resbox", F64] = kc.fused_kinds_module("f64", ((0, 0), (34, 70)), ((1, 1), (33, 69)), ((4, 4), (30, 66)), kc._residual_body("f64"), 1,
                                             KINDS)
    return t


TEXTS = _texts()


@pytest.fixture(scope="module")
def nh(built_libs):
    import torch
    assert torch.cuda.is_available()
    from neptune_hip import _capi, apply, fields
    _capi.load().neptune_hip_init(0)

    class NS:
        pass
    ns = NS()
    ns.capi, ns.apply, ns.fields, ns.torch = _capi, apply, fields, torch
    return ns


@pytest.fixture(scope="module")
def mods(nh, tmp_path_factory):
    """every module of this file, compiled up front in parallel into a cache of its own"""
    import os
    from neptune_hip import lowering
    old = os.environ.get("NEPTUNE_CACHE_DIR")
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("reduce_kinds_cache"))
    helpers.prefetch_modules(list(TEXTS.values()))
    cache = {}

    def get(*key):
        if key not in cache:
            cache[key] = lowering.compile_module(TEXTS[key])
        return cache[key]
    yield get
    if old is None:
        os.environ.pop("NEPTUNE_CACHE_DIR", None)
    else:
        os.environ["NEPTUNE_CACHE_DIR"] = old


def _bits(v, dt):
    a = np.asarray(dt(v))
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]).item()


def _same(got, want, dt):
    """got: the double an entry returns -- the element-type result widened, so casting it back is exact"""
    if math.isnan(float(want)):
        return math.isnan(got)
    assert float(dt(got)) == got
    return _bits(got, dt) == _bits(want, dt)


def _data(shape, dt, seed):
    return helpers.hash_field(shape, dt, seed=seed)


def _cases(dt, idle=False):
    for shape, lb, boxes in SHAPES[dt] + (IDLE[dt] if idle else []):
        for box in boxes:
            yield shape, lb, box


def _logical(lb, box):
    if box is None:
        return None
    return tuple(l + o for l, o in zip(box[0], lb)), tuple(h + o for h, o in zip(box[1], lb))


def _field(nh, x, lb):
    return nh.fields.DeviceField.from_numpy(x, lb)


def _cells(x, box):
    return x[rc.box_slices(box, x.ndim)]


def test_the_shapes_cover_idle_workgroups_and_dead_slots():
    """the case list itself, from the host's launch arithmetic: for each first-pass kernel of the plain reduce and each
    dtype some case has a workgroup with no work at all (not the last one, which takes the flat kernel's scalar tail), the
    table's n = 3 has an empty vector run, and the box kernel has a trip with dead unroll slots"""
    for dt in DTYPES:
        v = rc.VK[np.dtype(dt)]
        idle = {"flat": False, "box": False}
        empty_run = dead = False
        for shape, _, box in _cases(dt, idle=True):
            path = rc.plain_path(shape, box)
            ext = rc.box_ext(shape, box)
            blocks = rc.launch_blocks(path, dt, ext if path == "box" else (int(np.prod(shape)),))
            if path == "flat":
                units = int(np.prod(shape)) // v
                empty_run |= units == 0
            else:
                units = int(np.prod(ext[:-1])) * -(-ext[-1] // (256 * v))
                dead |= units % 4 != 0
            per = -(-units // blocks) if units else 0
            idle[path] |= blocks >= 2 and (blocks - 2) * per >= units
        assert idle["flat"] and idle["box"] and dead and (empty_run or dt is F64), (dt, idle, dead, empty_run)


@pytest.mark.parametrize("dt", DTYPES)
def test_identity_does_not_leak(nh, dt):
    """max over all-negative cells, min over all-positive ones: a 0 from a dead slot, a tail lane or an idle workgroup
    would win"""
    for shape, lb, box in _cases(dt, idle=True):
        neg = (-(dt(1) + np.abs(_data(shape, dt, 11)))).astype(dt)
        f = _field(nh, neg, lb)
        got = nh.apply.reduce(f, "max", _logical(lb, box))
        assert _same(got, kc.np_max(_cells(neg, box)), dt), (shape, box, got)
        f = _field(nh, -neg, lb)
        got = nh.apply.reduce(f, "min", _logical(lb, box))
        assert _same(got, kc.np_min(_cells(-neg, box)), dt), (shape, box, got)


def _positions(shape, box, dt, rng):
    """first cell, last cell, every row's last cell and the lanes of its partial vector, 32 seeded cells (array indices
    inside the reduced box)"""
    lo, hi = box if box is not None else ((0,) * len(shape), tuple(shape))
    ext = tuple(h - l for l, h in zip(lo, hi))
    v = rc.VK[np.dtype(dt)]
    pos = {tuple(lo), tuple(h - 1 for h in hi)}
    tail = range(max(0, ext[-1] - max(ext[-1] % v, 1) - 1), ext[-1])
    for row in np.ndindex(*ext[:-1]):
        for k in tail:
            pos.add(tuple(l + r for l, r in zip(lo, row)) + (lo[-1] + k,))
    for _ in range(32):
        pos.add(tuple(int(rng.integers(l, h)) for l, h in zip(lo, hi)))
    return sorted(pos)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_extreme_anywhere_is_found(nh, dt):
    rng = np.random.default_rng(5)
    for shape, lb, box in _cases(dt):
        x = _data(shape, dt, 12)            # cells in [-1, 1)
        f = _field(nh, x, lb)
        lbox = _logical(lb, box)
        for p in _positions(shape, box, dt, rng):
            old = float(x[p])
            for kind, val in (("max", 5.0), ("min", -5.0)):
                f.tensor[p] = val
                got = nh.apply.reduce(f, kind, lbox)
                assert _same(got, dt(val), dt), (shape, box, p, kind, got)
            f.tensor[p] = old
        assert _same(nh.apply.reduce(f, "max", lbox), kc.np_max(_cells(x, box)), dt)
        assert _same(nh.apply.reduce(f, "min", lbox), kc.np_min(_cells(x, box)), dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_nan_inside_poisons_and_nan_outside_does_not(nh, dt):
    for shape, lb, box in _cases(dt):
        x = _data(shape, dt, 13)
        lo, hi = box if box is not None else ((0,) * len(shape), tuple(shape))
        spots = [tuple(lo), tuple(h - 1 for h in hi), tuple(lo[:-1]) + (hi[-1] - 1,)]   # first cell, last cell, a row's tail
        for p in spots:
            y = x.copy()
            y[p] = np.nan
            f = _field(nh, y, lb)
            for kind in KINDS:
                assert math.isnan(nh.apply.reduce(f, kind, _logical(lb, box))), (shape, box, p, kind)
        if box is not None:
            y = np.full(shape, np.nan, dt)
            y[rc.box_slices(box, len(shape))] = _cells(x, box)
            f = _field(nh, y, lb)
            cells = _cells(x, box)
            for kind in ("max", "min"):
                assert _same(nh.apply.reduce(f, kind, _logical(lb, box)), kc.np_kind(kind, cells), dt), (shape, box, kind)
            flat = cells.reshape(-1)
            n, eps = flat.size, float(np.finfo(dt).eps)
            d1 = 2 * (n - 1) * eps * float(np.abs(flat).astype(np.float64).sum())
            d2 = 2 * (n - 1) * eps * float((flat * flat).astype(np.float64).sum())
            l1, l2 = (nh.apply.reduce(f, kind, _logical(lb, box)) for kind in ("l1", "l2"))
            assert abs(l1 - float(kc.np_kind("l1", flat))) <= d1, (shape, box, l1)
            ser2 = float(kc.serial_sum(flat * flat))
            assert abs(l2 - float(np.sqrt(dt(ser2)))) <= d2 / math.sqrt(ser2) + eps * math.sqrt(ser2), (shape, box, l2)


@pytest.mark.parametrize("dt", DTYPES)
def test_signed_zeros(nh, dt):
    for shape, lb, box in _cases(dt):
        z = np.full(shape, -0.0, dt)
        f = _field(nh, z, lb)
        got = nh.apply.reduce(f, "max", _logical(lb, box))
        assert got == 0 and math.copysign(1, got) < 0, (shape, box, "all -0: max = -0")
        lo, hi = box if box is not None else ((0,) * len(shape), tuple(shape))
        for p in (tuple(lo), tuple(h - 1 for h in hi)):
            z2 = z.copy()
            z2[p] = 0.0
            f = _field(nh, z2, lb)
            gmax, gmin = (nh.apply.reduce(f, k, _logical(lb, box)) for k in ("max", "min"))
            assert gmax == 0 and math.copysign(1, gmax) > 0, (shape, box, p)
            assert gmin == 0 and math.copysign(1, gmin) < 0, (shape, box, p)


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_bounds_give_the_identity(nh, dt):
    x = _data((5, 7), dt, 14)
    f = _field(nh, x, (-2, 3))
    for kind, want in (("max", -np.inf), ("min", np.inf), ("l1", 0.0), ("l2", 0.0), ("sum", 0.0)):
        for empty in (((0, 5), (0, 9)), ((-1, 6), (2, 6))):
            got = nh.apply.reduce(f, kind, empty)
            assert got == want and math.copysign(1, got) == math.copysign(1, want), (kind, empty, got)


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_bounds_in_lowered_modules(nh, mods, dt):
    """the early returns of run_reduce (rank 2, rank 4 bounded) and of the fused form: the kind's identity, nothing read"""
    want = {"max": -np.inf, "min": np.inf, "l1": 0.0, "l2": 0.0, "sum": 0.0}
    nan2 = np.full(tuple(h - l for l, h in zip(*BOX2)), np.nan, dt)
    nan4 = np.full(RANK4[0], np.nan, dt)
    nanp = np.full(PW_SHAPE[dt], np.nan, dt)
    for kind in kc.ALL_KINDS:
        for got in (mods("p2", dt).call(f"{kind}_2", nan2), mods("p4", dt).call(f"{kind}_3", nan4),
                    mods("pwempty", dt).call(kind, nanp, nanp)):
            assert got == want[kind] and math.copysign(1, got) == math.copysign(1, want[kind]), (kind, got)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank4_extremes_zeros_and_the_flat_tree(nh, mods, dt):
    """rank 4 through the lowered module: a lone extreme anywhere (whole buffer and bounded box), signed zeros, and the
    whole-buffer l1 / l2 bit-equal to reduce_sum of |x| / x*x over the same flat buffer (one flat pass, the sum's tree)"""
    shape, boxes = RANK4
    mod = mods("p4", dt)
    rng = np.random.default_rng(6)
    x = _data(shape, dt, 31)
    for i in (0, 2):
        lo, hi = boxes[i] if boxes[i] is not None else ((0,) * 4, shape)
        pos = {tuple(lo), tuple(h - 1 for h in hi)}
        pos |= {(a, b, c, hi[3] - 1 - k) for a in range(lo[0], hi[0]) for b, c in ((lo[1], lo[2]), (hi[1] - 1, hi[2] - 1)) for k in range(3)}
        pos |= {tuple(int(rng.integers(l, h)) for l, h in zip(lo, hi)) for _ in range(8)}
        for p in sorted(pos):
            y = x.copy()
            y[p] = 5.0
            assert _same(mod.call(f"max_{i}", y), dt(5.0), dt), (i, p)
            y[p] = -5.0
            assert _same(mod.call(f"min_{i}", y), dt(-5.0), dt), (i, p)
        z = np.full(shape, -0.0, dt)
        got = mod.call(f"max_{i}", z)
        assert got == 0 and math.copysign(1, got) < 0, i
        z[tuple(h - 1 for h in hi)] = 0.0
        gmax, gmin = mod.call(f"max_{i}", z), mod.call(f"min_{i}", z)
        assert gmax == 0 and math.copysign(1, gmax) > 0 and gmin == 0 and math.copysign(1, gmin) < 0, i
    flat = _field(nh, x.reshape(-1), (0,))
    fabs = nh.fields.DeviceField(flat.lb, flat.ub, flat.dtype, nh.torch.abs(flat.tensor))
    fsq = nh.fields.DeviceField(flat.lb, flat.ub, flat.dtype, flat.tensor * flat.tensor)
    assert _same(mod.call("l1_0", x), dt(nh.apply.reduce_sum(fabs)), dt)
    assert _same(mod.call("l2_0", x), np.sqrt(dt(nh.apply.reduce_sum(fsq))), dt)
    assert _same(mod.call("sum_0", x), dt(nh.apply.reduce_sum(flat)), dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_l1_and_l2_run_on_the_tree_of_sum(nh, dt):
    """no tolerance: |f| and f*f made by torch in the element type, summed by reduce_sum on the same box"""
    n_eps = float(np.finfo(dt).eps)
    for shape, lb, box in _cases(dt, idle=True):
        x = _data(shape, dt, 15)
        f = _field(nh, x, lb)
        lbox = _logical(lb, box)
        fabs = nh.fields.DeviceField(f.lb, f.ub, f.dtype, nh.torch.abs(f.tensor))
        fsq = nh.fields.DeviceField(f.lb, f.ub, f.dtype, f.tensor * f.tensor)
        l1, l2 = nh.apply.reduce(f, "l1", lbox), nh.apply.reduce(f, "l2", lbox)
        s_abs, s_sq = nh.apply.reduce_sum(fabs, lbox), nh.apply.reduce_sum(fsq, lbox)
        assert _same(l1, dt(s_abs), dt), (shape, box)
        assert _same(l2, np.sqrt(dt(s_sq)), dt), (shape, box)
        assert _same(nh.apply.reduce(f, nh.capi.REDUCE_L2 | nh.capi.REDUCE_RAW, lbox), dt(s_sq), dt), (shape, box)
        # against a serial NumPy sum in the element type: the bound of the sum, 2 (n - 1) eps sum|t_i|
        cells = _cells(x, box).reshape(-1)
        n = cells.size
        t1, t2 = np.abs(cells), cells * cells
        d1 = 2 * (n - 1) * n_eps * float(np.sum(t1.astype(np.float64)))
        d2 = 2 * (n - 1) * n_eps * float(np.sum(t2.astype(np.float64)))
        ser1, ser2 = float(kc.serial_sum(t1)), float(kc.serial_sum(t2))
        print(f"{shape} {box}: l1 {l1!r} serial {ser1!r} bound {d1:.3e}; sumsq {s_sq!r} serial {ser2!r} bound {d2:.3e}; l2 {l2!r}")
        assert abs(l1 - ser1) <= d1 and abs(s_sq - ser2) <= d2, (shape, box)
        # l2: |sqrt(S) - sqrt(S')| <= |S - S'| / sqrt(S'), plus one rounding of each sqrt
        root = math.sqrt(ser2)
        assert abs(l2 - float(np.sqrt(dt(ser2)))) <= d2 / root + n_eps * root, (shape, box)


@pytest.mark.parametrize("dt", DTYPES)
def test_l2_of_threes_and_fours_is_exact(nh, dt):
    for shape, lb, box in _cases(dt):
        lo, hi = box if box is not None else ((0,) * len(shape), tuple(shape))
        ext = tuple(h - l for l, h in zip(lo, hi))
        n = int(np.prod(ext))
        m = int(math.isqrt(n // 2))
        if m == 0:
            continue
        x = np.full(shape, 7.0, dt)                     # outside the box: must not count
        cells = np.zeros(n, dt)
        cells[: m * m] = 3.0                            # m^2 threes and m^2 fours: sum x^2 = 25 m^2, every partial sum exact
        cells[m * m: 2 * m * m] = 4.0
        np.random.default_rng(3).shuffle(cells)
        x[rc.box_slices(box, len(shape))] = cells.reshape(ext)
        f = _field(nh, x, lb)
        assert nh.apply.reduce(f, "l2", _logical(lb, box)) == 5.0 * m, (shape, box)
        assert nh.apply.reduce(f, "l1", _logical(lb, box)) == 7.0 * m * m, (shape, box)


@pytest.mark.parametrize("dt", DTYPES)
def test_lowered_plain_reduces(nh, mods, dt):
    """rank 2 and 3 through a lowered module: the bits of apply.reduce; every kind, whole field and sub-box"""
    for key, (lbx, sub) in (("p2", (BOX2, SUB2)), ("p3", (BOX3, SUB3))):
        shape = tuple(h - l for l, h in zip(*lbx))
        mod = mods(key, dt)
        for seed, sign in ((16, 1), (17, -1)):
            x = _data(shape, dt, seed)
            x = (sign * (dt(1) + np.abs(x))).astype(dt) if sign < 0 else x
            f = _field(nh, x, lbx[0])
            for i, red in enumerate((None, sub)):
                for kind in kc.ALL_KINDS:
                    got = mod.call(f"{kind}_{i}", x)
                    assert _same(got, dt(nh.apply.reduce(f, kind, red)), dt), (key, kind, red)
                    if kind in ("max", "min"):
                        arr = None if red is None else tuple(tuple(v - o for v, o in zip(b, lbx[0])) for b in red)
                        assert _same(got, kc.np_kind(kind, _cells(x, arr)), dt), (key, kind, red)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank4_whole_and_bounded(nh, mods, dt):
    """whole buffer: one flat pass; bounded: per-leading-index results combined with the kind's own combine -- for l2 the
    sums of squares are added and one sqrt is taken"""
    shape, boxes = RANK4
    mod = mods("p4", dt)
    for seed, neg in ((18, False), (19, True)):
        x = _data(shape, dt, seed)
        if neg:
            x = (-(dt(1) + np.abs(x))).astype(dt)
        for i, box in enumerate(boxes[:3]):
            cells = _cells(x, box)
            assert _same(mod.call(f"max_{i}", x), kc.np_max(cells), dt), (i, "max")
            assert _same(mod.call(f"min_{i}", -x), kc.np_min(-cells), dt), (i, "min")
            n, eps = cells.size, float(np.finfo(dt).eps)
            t1, t2 = np.abs(cells).reshape(-1), (cells * cells).reshape(-1)
            d1 = 2 * (n - 1) * eps * float(np.sum(t1.astype(np.float64)))
            d2 = 2 * (n - 1) * eps * float(np.sum(t2.astype(np.float64)))
            ser2 = float(kc.serial_sum(t2))
            assert abs(mod.call(f"l1_{i}", x) - float(kc.serial_sum(t1))) <= d1, (i, "l1")
            assert abs(mod.call(f"l2_{i}", x) - float(np.sqrt(dt(ser2)))) <= d2 / math.sqrt(ser2) + eps * math.sqrt(ser2), (i, "l2")
        y = np.full(shape, np.nan, dt)                      # NaN everywhere outside the bounded box
        y[rc.box_slices(boxes[2], 4)] = _cells(x, boxes[2])
        assert _same(mod.call("max_2", y), kc.np_max(_cells(x, boxes[2])), dt)
        assert math.isfinite(mod.call("l2_2", y))
        y = x.copy()
        y[1, 2, 2, 68] = np.nan                             # the last cell of the bounded box
        for kind in KINDS:
            assert math.isnan(mod.call(f"{kind}_2", y)), kind
    # small integers: 3s and 4s over the bounded box, exact whatever the order
    lo, hi = boxes[2]
    ext = tuple(h - l for l, h in zip(lo, hi))
    n = int(np.prod(ext))
    m = int(math.isqrt(n // 2))
    cells = np.zeros(n, dt)
    cells[: m * m], cells[m * m: 2 * m * m] = 3.0, 4.0
    x = np.full(shape, 9.0, dt)
    x[rc.box_slices(boxes[2], 4)] = cells.reshape(ext)
    assert mod.call("l2_2", x) == 5.0 * m


def test_fused_residual_max_norm(nh, mods):
    """|A(u) - u| on 34 x 70, apply.bounds the interior, the reduce over the whole box: the non-vector kernel.  The rim
    is copy-through, so input 0 itself is folded in there"""
    mod = mods("res", F64)
    assert rc.fused_path(F64, False, (34, 70), (0, 0), (34, 70), True) == "fused_scalar"
    base = (helpers.hash_field((34, 70), F64, seed=21) * 0.125).astype(F64)
    # 1. the max lies in an interior cell
    u = base.copy()
    u[17, 33] = 3.0
    r = kc.np_residual(u)
    assert np.unravel_index(np.argmax(r), r.shape) == (17, 33)
    for kind in ("max", "min"):
        assert _same(mod.call(kind, u), kc.np_kind(kind, r), F64), kind
    # 2. ... in a copy-through rim cell (no interior cell's footprint reads a corner)
    u = base.copy()
    u[33, 69] = 7.0
    r = kc.np_residual(u)
    assert r.max() == 7.0 and np.unravel_index(np.argmax(r), r.shape) == (33, 69)
    assert _same(mod.call("max", u), F64(7.0), F64)
    u[0, 0] = -9.0
    assert _same(mod.call("min", u), F64(-9.0), F64)
    # 3. plain data: the rim holds cells of both signs, the interior residuals are >= 0
    u = base.copy()
    r = kc.np_residual(u)
    for kind in KINDS[:2]:
        assert _same(mod.call(kind, u), kc.np_kind(kind, r), F64), kind
    n, eps = r.size, float(np.finfo(F64).eps)
    assert abs(mod.call("l1", u) - float(kc.serial_sum(np.abs(r)))) <= 2 * (n - 1) * eps * float(np.abs(r).sum())
    ser2 = float(kc.serial_sum(r.reshape(-1) * r.reshape(-1)))
    d2 = 2 * (n - 1) * eps * float((r * r).sum())
    assert abs(mod.call("l2", u) - math.sqrt(ser2)) <= d2 / math.sqrt(ser2) + eps * math.sqrt(ser2)
    # 4. NaN in a cell that counts poisons every kind: an interior neighbour, a rim cell
    for p in ((5, 5), (0, 40)):
        v = base.copy()
        v[p] = np.nan
        for kind in KINDS:
            assert math.isnan(mod.call(kind, v)), (p, kind)


def test_fused_residual_ignores_a_nan_no_counted_cell_reads(nh, mods):
    """the reduce restricted to a box whose cells' footprints stay clear of the NaN cells: a halo-read cell outside every
    counted cell's footprint must not reach the result"""
    mod = mods("resbox", F64)     # apply.bounds the interior, the reduce over [4, 30) x [4, 66)
    u = (helpers.hash_field((34, 70), F64, seed=22) * 0.125).astype(F64)
    r = kc.np_residual(u)[4:30, 4:66]
    v = u.copy()
    v[:3, :] = np.nan          # rows the counted cells' footprints (rows 3..30) never read
    v[31:, :] = np.nan
    v[:, :3] = np.nan
    v[:, 67:] = np.nan
    v[3, 3] = v[30, 66] = np.nan   # the corners next to the box: no 5-point footprint of a counted cell holds them
    for kind in ("max", "min"):
        assert _same(mod.call(kind, v), kc.np_kind(kind, r), F64), kind
    for kind in ("l1", "l2"):
        assert _same(mod.call(kind, v), F64(mod.call(kind, u)), F64), kind


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_pointwise_takes_the_vector_kernel(nh, mods, dt):
    shape = PW_SHAPE[dt]
    assert rc.fused_path(dt, True, shape, (0, 0), shape, True) == "fused_vec"
    mod = mods("pw", dt)
    a = (-(dt(2) + np.abs(_data(shape, dt, 23)))).astype(dt)
    b = _data(shape, dt, 24)
    d = np.abs(a - b)
    assert _same(mod.call("max", a, b), kc.np_max(d), dt) and _same(mod.call("min", a, b), kc.np_min(d), dt)
    # a lone extreme in every lane position of the last vector of a row, and in the first cell
    for p in [(0, 0)] + [(shape[0] - 1, shape[1] - 1 - k) for k in range(rc.VK[np.dtype(dt)])] + [(3, shape[1] - 1)]:
        a2 = a.copy()
        a2[p] = 50.0
        assert _same(mod.call("max", a2, b), kc.np_max(np.abs(a2 - b)), dt), p
        a2[p] = b[p]
        assert _same(mod.call("min", a2, b), dt(0.0), dt), p
        a2[p] = np.nan
        for kind in KINDS:
            assert math.isnan(mod.call(kind, a2, b)), (p, kind)
    n, eps = d.size, float(np.finfo(dt).eps)
    assert abs(mod.call("l1", a, b) - float(kc.serial_sum(d))) <= 2 * (n - 1) * eps * float(d.astype(np.float64).sum())


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_l1_and_l2_are_the_fused_sum_of_the_mapped_body(nh, mods, dt):
    """reduce bounds inside apply.bounds: l1 / l2 of the body d equal, bit for bit, the fused sum of a module whose body
    computes |d| resp. d*d itself (same kernel, same tree); l2 takes one correctly rounded sqrt of it"""
    shape = PW_SHAPE[dt]
    a, b = _data(shape, dt, 25), _data(shape, dt, 26)
    mid, mabs, msq = mods("id", dt), mods("abs", dt), mods("sq", dt)
    assert _same(mid.call("l1", a, b), dt(mabs.call("sum", a, b)), dt)
    assert _same(mid.call("l2", a, b), np.sqrt(dt(msq.call("sum", a, b))), dt)
    red = INNER[dt][1]
    d = (a - b)[rc.box_slices(red, 2)]
    n, eps = d.size, float(np.finfo(dt).eps)
    assert abs(mid.call("l1", a, b) - float(kc.serial_sum(np.abs(d)))) <= 2 * (n - 1) * eps * float(np.abs(d).astype(np.float64).sum())


def test_reproducible_and_refusals(nh, mods):
    import ctypes as C
    lib = nh.capi.load()
    x = _data((33, 1030), F32, 27)
    f = _field(nh, x, (0, 0))
    for box in (None, ((0, 0), (33, 1029))):
        for kind in kc.ALL_KINDS:
            r1, r2 = nh.apply.reduce(f, kind, box), nh.apply.reduce(f, kind, box)
            assert _bits(r1, F32) == _bits(r2, F32), (kind, box)
        assert _bits(nh.apply.reduce(f, "sum", box), F32) == _bits(nh.apply.reduce_sum(f, box), F32), box
        assert _bits(nh.apply.reduce(f, nh.capi.REDUCE_SUM | nh.capi.REDUCE_RAW, box), F32) == _bits(nh.apply.reduce_sum(f, box), F32)
    arr = lambda v: (C.c_int64 * 2)(*v)
    out = C.c_double(123.0)
    for bad in (5, -1, 99, nh.capi.REDUCE_RAW | 7):
        rc_ = lib.neptune_hip_reduce(bad, f.dtype, 2, f.ptr, arr(f.lb), arr(f.ub), None, None, C.byref(out), None)
        assert rc_ == nh.capi.EINVAL and out.value == 123.0, bad
    for kind in range(5):
        rc_ = lib.neptune_hip_reduce(kind, f.dtype, 2, f.ptr, arr(f.lb), arr(f.ub), arr((0, 0)), arr((34, 10)), C.byref(out), None)
        assert rc_ == nh.capi.EOOB and out.value == 123.0, kind
    with pytest.raises(ValueError, match="unknown reduce kind"):
        nh.apply.reduce(f, "prod")
