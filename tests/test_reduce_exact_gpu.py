"""neptune_ir.reduce {kind = "sum"} on the device, pinned to exact sums and to the tree-height error bound.

Every assertion here is one of three kinds:
  * bit equality with reduce_cases.exact_sum on exact data (integer multiples of one power of two with
    sum|x| <= 2^p): every summation order returns the exact sum, so every cell counts;
  * an identity of special values (NaN, +-Inf, signed zeros, subnormals);
  * |got - fsum| <= gamma_h sum|x| on general data, h = reduce_cases.tree_height of the launch the host makes.
Cells a correct kernel never reads hold NaN (reduce_cases.*_sentinel_mask), so an over-read shows as a NaN result.

Paths (kernel <- host entry): neptune_reduce_partial_flat and neptune_reduce_partial_box <- neptune_hip_reduce_sum;
neptune_reduce_apply and neptune_reduce_apply_vec <- run_apply_reduce_sum (lowered reduce of a single-use apply);
rank 4..6 <- run_reduce_sum (the flat kernel on the whole buffer, or one rank-3 box sum per leading index)."""
import math

import numpy as np
import pytest

import helpers
import reduce_cases as rc
from helpers import oracle

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]
ELEM = {F64: "f64", F32: "f32"}
NAN = float("nan")


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
def lower(nh, tmp_path_factory):
    """compile_module into a cache of this module's own; every module text below is compiled up front in parallel"""
    import os
    from neptune_hip import lowering
    old = os.environ.get("NEPTUNE_CACHE_DIR")
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("reduce_exact_cache"))
    texts = [c.text for c in FUSED_EXACT + FUSED_SPECIAL] + [c.text for c in FUSED_GAMMA] + [c.text for c in FUSED_HUGE]
    texts += [rc.plain_module(ELEM[dt], box, red) for dt in DTYPES for box, red in LOWERED_PLAIN]
    texts += [rc.plain_module(ELEM[dt], box, red) for dt in DTYPES for box, red in RANK_N]
    texts += [rc.plain_module(ELEM[dt], box, _empty(red if red is not None else box))
              for dt in DTYPES for box, red in LOWERED_PLAIN + RANK_N]
    texts += [rc.plain_module("f32", ((0,) * 4, (3, 2, 4, 8)), ((0, 0, 0, 0), (3, 2, 4, 8)))]
    helpers.prefetch_modules(texts)
    cache = {}

    def get(text):
        if text not in cache:
            cache[text] = lowering.compile_module(text)
        return cache[text]
    yield get
    if old is None:
        os.environ.pop("NEPTUNE_CACHE_DIR", None)
    else:
        os.environ["NEPTUNE_CACHE_DIR"] = old


def _bits(v, dt):
    a = np.asarray(dt(v))
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]).item()


def _same(got, want, dt):
    """got: the double the host entry returns; for f32 it is the f32 result widened, so the cast back is exact"""
    assert float(dt(got)) == got or math.isnan(got)
    return _bits(got, dt) == _bits(want, dt)


# ---- plain reduce: neptune_hip_reduce_sum --------------------------------------------------------------------------
def _plain_sum(nh, x, box=None, misalign=False):
    """reduce x (numpy) over box (array indices, None = whole buffer) on the device; misalign: the buffer starts one
    element past a 16-byte boundary (a torch view at element offset 1), which forces the box kernel"""
    torch = nh.torch
    t = torch.from_numpy(np.ascontiguousarray(x).reshape(-1))
    if misalign:
        base = torch.empty(x.size + 4, dtype=t.dtype, device="cuda")
        dev = base[1:1 + x.size]
        dev.copy_(t.cuda())
        assert dev.data_ptr() % 16 != 0
    else:
        dev = t.cuda()
    dev = dev.view(x.shape)
    f = nh.fields.DeviceField((0,) * x.ndim, x.shape, nh.capi.F64 if x.dtype == F64 else nh.capi.F32, tensor=dev)
    return nh.apply.reduce_sum(f, box)


def _vk(dt):
    return rc.VK[np.dtype(dt)]


def _flat_counts(dt):
    v = _vk(dt)
    big = 256 * v * rc.K_REDUCE_BLOCKS
    # 600_001 % VK != 0 and > 256 * 2048 cells: 2048 workgroups, the scalar tail on lane 0 of the last one
    return [1, v - 1, v + 1, 255, 257, big - 1, big, big + 1, 600_001]


def _box_cases(dt):
    v = _vk(dt)
    cases = []
    for row in (1, v - 1, 256 * v, 256 * v + 1, 3 * 256 * v + v + 1):
        cases.append(((7, row + 3), ((1, 2), (6, row + 2))))
    cases += [
        ((4098, 5), ((1, 1), (4097, 4))),                   # 4096 rows of 3
        ((1000,), ((3,), (997,))),                           # rank 1
        ((37, 129), ((5, 0), (30, 100))),                    # rank 2
        ((20, 33, 65), ((2, 5, 7), (19, 30, 60))),           # rank 3
        ((9, 9, 9), ((4, 4, 4), (5, 5, 5))),                 # one cell
    ]
    for chunks in (4 * 2048 - 1, 4 * 2048, 4 * 2048 + 1):    # one chunk per row: the 2048-workgroup cap +- 1 chunk
        cases.append(((chunks + 2, 40), ((1, 3), (chunks + 1, 37))))
    # rank 3, three chunks per row (the last one ragged), 2731 rows: 8193 chunks
    cases.append(((3, 2733, 2 * 256 * v + 5), ((1, 1, 1), (2, 2732, 2 * 256 * v + 4))))
    return cases


@pytest.mark.parametrize("dt", DTYPES)
def test_flat_reduce_is_exact(nh, dt):
    for n in _flat_counts(dt):
        x = rc.exact_field((n,), dt, seed=n)
        assert rc.plain_path(x.shape, None) == "flat"
        got = _plain_sum(nh, x)
        assert _same(got, rc.exact_sum(x), dt), (n, got, rc.exact_sum(x))


@pytest.mark.parametrize("dt", DTYPES)
def test_box_reduce_is_exact_with_nan_outside_the_box(nh, dt):
    for shape, box in _box_cases(dt):
        x = rc.exact_field(shape, dt, seed=len(shape) * 1000 + shape[-1])
        want = rc.exact_sum(x, box)
        x[rc.plain_sentinel_mask(shape, box)] = NAN
        assert rc.plain_path(shape, box) == "box"
        got = _plain_sum(nh, x, box)
        assert _same(got, want, dt), (shape, box, got, want)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [5, 1001, 600_001])
def test_misaligned_whole_buffer_takes_the_box_kernel_and_is_exact(nh, dt, n):
    x = rc.exact_field((n,), dt, seed=7)
    assert rc.plain_path(x.shape, None, aligned=False) == "box"
    assert _same(_plain_sum(nh, x, misalign=True), rc.exact_sum(x), dt)
    x2 = rc.exact_field((3, n), dt, seed=8)
    assert _same(_plain_sum(nh, x2, misalign=True), rc.exact_sum(x2), dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_plain_reduce_of_subnormal_data_is_exact(nh, dt):
    sub = -1074 if dt == F64 else -149
    for shape, box in [((600_001,), None), ((37, 129), ((5, 0), (30, 100))), ((1001,), None)]:
        x = rc.exact_field(shape, dt, seed=3, scale_exp=sub)
        want = rc.exact_sum(x, box)
        assert want != 0
        if box is not None:
            x[rc.plain_sentinel_mask(shape, box)] = NAN
        for mis in ((False, True) if box is None else (False,)):
            assert _same(_plain_sum(nh, x, box, misalign=mis), want, dt), (shape, mis)


@pytest.mark.parametrize("max_abs", [1 << 20, 1 << 30])
def test_plain_reduce_of_f64_data_needing_more_than_24_bits_is_exact(nh, max_abs):
    """an accumulator narrower than f64 rounds these partial sums (2^20) or the cells themselves (2^30)"""
    for n in (100_000, 1_000_003):
        x = rc.exact_field((n,), F64, seed=9, max_abs=max_abs)
        for mis in (False, True):
            assert _same(_plain_sum(nh, x, misalign=mis), rc.exact_sum(x), F64), (n, mis)
    y = rc.exact_field((101, 1003), F64, seed=10, max_abs=max_abs)
    assert _same(_plain_sum(nh, y, ((1, 1), (100, 1002))), rc.exact_sum(y, ((1, 1), (100, 1002))), F64)


def _special_plain_cases(dt):
    """(x, box, expected) triples: NaN anywhere that counts -> NaN; +Inf -> +Inf; +Inf and -Inf -> NaN"""
    v = _vk(dt)
    out = []
    for n in (600_001, 257, v + 1):                        # flat, each with a scalar tail
        for pos in (0, n - 1, n - n % v, n // 2):             # first, last, first of the tail, middle
            x = rc.exact_field((n,), dt, seed=n)
            x[pos] = NAN
            out.append((f"flat n={n} NaN@{pos}", x, None, "nan"))
    row = 256 * v + v + 1                                 # ragged rows: the last, partial vector of a row
    shape, box = (9, row + 2), ((1, 1), (8, row + 1))
    for cell in ((1, 1), (7, row), (4, row), (4, row - 1)):
        x = rc.exact_field(shape, dt, seed=1)
        x[rc.plain_sentinel_mask(shape, box)] = 0
        x[cell] = NAN
        out.append((f"box NaN@{cell}", x, box, "nan"))
    for path_box, shape in ((None, (600_001,)), (((1, 1), (8, row + 1)), (9, row + 2))):
        x = np.zeros(shape, dt)
        x.reshape(-1)[-1 if path_box is None else (7 * (row + 2) + row)] = np.inf
        out.append(("+inf", x.copy(), path_box, "+inf"))
        x.reshape(-1)[1 if path_box is None else (row + 2 + 1)] = -np.inf
        out.append(("+inf -inf", x, path_box, "nan"))
    return out


@pytest.mark.parametrize("dt", DTYPES)
def test_plain_reduce_special_values(nh, dt):
    for name, x, box, want in _special_plain_cases(dt):
        for mis in ((False, True) if box is None else (False,)):
            got = _plain_sum(nh, x, box, misalign=mis)
            if want == "nan":
                assert math.isnan(got), (name, mis, got)
            else:
                assert got == math.inf, (name, mis, got)
    # all -0.0: +0.0 bits on both kernels; an empty box: +0.0 without a launch
    for shape, box in (((600_001,), None), ((37, 129), ((5, 0), (30, 100))), ((1001,), None)):
        z = np.full(shape, -0.0, dt)
        for mis in ((False, True) if box is None else (False,)):
            assert _bits(_plain_sum(nh, z, box, misalign=mis), dt) == 0
    z = np.full((8, 8), NAN, dt)
    assert _bits(_plain_sum(nh, z, ((3, 3), (3, 8))), dt) == 0


# ---- plain reduce through the lowering: run_reduce_sum, ranks 1..6 ------------------------------------------------
LOWERED_PLAIN = [
    (((0,), (5000,)), ((1,), (4999,))),
    (((-2, 3), (40, 300)), ((0, 4), (39, 299))),
    (((0, 0, 0), (9, 7, 300)), ((0, 1, 1), (9, 5, 298))),
]
# odd cell counts: the whole-buffer sums have a scalar tail in f64 and in f32
RANK_N = [
    (((0,) * 4, (3, 5, 7, 131)), None),                             # flat kernel on the whole buffer
    (((0,) * 4, (3, 5, 7, 131)), ((1, 1, 0, 3), (3, 5, 6, 130))),   # one rank-3 box sum per leading index
    (((0,) * 5, (3, 3, 5, 7, 71)), None),
    (((0,) * 5, (3, 3, 5, 7, 71)), ((0, 1, 1, 1, 1), (2, 3, 4, 5, 70))),
    (((0,) * 6, (3, 1, 3, 5, 5, 67)), None),
    (((0,) * 6, (3, 1, 3, 5, 5, 67)), ((1, 0, 1, 0, 1, 2), (3, 1, 3, 4, 4, 66))),
]


def _empty(box):
    """the box with its first axis cut to zero extent"""
    return box[0], (box[0][0],) + tuple(box[1][1:])


def _arr_box(box, red):
    if red is None:
        return None
    return tuple(l - o for l, o in zip(red[0], box[0])), tuple(h - o for h, o in zip(red[1], box[0]))


@pytest.mark.parametrize("dt", DTYPES)
def test_lowered_plain_reduce_is_exact_at_every_rank(nh, lower, dt):
    for box, red in LOWERED_PLAIN + RANK_N:
        shape = tuple(h - l for l, h in zip(*box))
        x = rc.exact_field(shape, dt, seed=len(shape))
        abox = _arr_box(box, red)
        want = rc.exact_sum(x, abox)
        if red is not None:
            x[rc.plain_sentinel_mask(shape, abox)] = NAN
        mod = lower(rc.plain_module(ELEM[dt], box, red))
        got = mod.call("red", nh.torch.from_numpy(x).cuda())
        assert _same(got, want, dt), (box, red, got, want)
        # special values: NaN at the first, last and middle cell of the box (on a whole buffer the last cell lies in
        # the flat kernel's scalar tail), +Inf alone, +Inf with -Inf, subnormals, -0.0
        run = lambda y: mod.call("red", nh.torch.from_numpy(y).cuda())   # noqa: E731
        lo = abox[0] if abox else (0,) * len(shape)
        hi = tuple(h - 1 for h in abox[1]) if abox else tuple(n - 1 for n in shape)
        assert int(np.prod(shape)) % _vk(dt) != 0 or abox is not None
        for cell in (lo, hi, tuple((l + h) // 2 for l, h in zip(lo, hi))):
            y = np.zeros(shape, dt)
            y[cell] = NAN
            assert math.isnan(run(y)), (box, red, cell)
        y = np.zeros(shape, dt)
        y[hi] = np.inf
        assert run(y) == math.inf
        y[lo] = -np.inf
        assert math.isnan(run(y))
        sub = -1074 if dt == F64 else -149
        s = rc.exact_field(shape, dt, seed=5, scale_exp=sub)
        assert _same(run(s), rc.exact_sum(s, abox), dt)
        assert _bits(run(np.full(shape, -0.0, dt)), dt) == 0
        # an empty box: +0.0 whatever the buffer holds
        empty = lower(rc.plain_module(ELEM[dt], box, _empty(red if red is not None else box)))
        assert _bits(empty.call("red", nh.torch.from_numpy(np.full(shape, NAN, dt)).cuda()), dt) == 0


def test_rank4_bounded_f32_reduce_adds_slab_sums_in_double(nh, lower):
    """Beyond rank 3 a bounded reduce is one rank-3 box sum per leading index; run_reduce_sum adds those sums on the host
    in double and rounds to f32 once.  That is intended: each kernel accumulates in the element type, as the comment in
    util_kernels.hpp says, and the host's wider accumulation of at most a few thousand slab sums only removes rounding.
    Slab sums 2^24, 1, -1: each slab is exact in f32, the total 2^24 is exact only with the wider accumulation (f32
    would give 2^24 + 1 -> 2^24, then 2^24 - 1)."""
    shape = (3, 2, 4, 8)
    box = ((0,) * 4, shape)
    red = ((0, 0, 0, 0), shape)
    x = np.zeros(shape, F32)
    x[0, 1, 2, 3], x[1, 0, 0, 7], x[2, 1, 3, 0] = 2.0 ** 24, 1.0, -1.0
    got = lower(rc.plain_module("f32", box, red)).call("red", nh.torch.from_numpy(x).cuda())
    assert _bits(got, F32) == _bits(2.0 ** 24, F32)
    f32_chain = np.float32(np.float32(np.float32(2.0 ** 24) + np.float32(1.0)) - np.float32(1.0))
    assert float(f32_chain) != 2.0 ** 24


# ---- fused reduce(apply): run_apply_reduce_sum ---------------------------------------------------------------------
class Fused:
    def __init__(self, elem, res_shape, bounds, red, in_boxes, body, path, div_zero=False, scale_exp=0):
        rank = len(res_shape)
        self.dt = F64 if elem == "f64" else F32
        self.res = ((0,) * rank, tuple(res_shape))
        self.bounds, self.red, self.body = bounds, red, body
        self.in_boxes = [self.res] + list(in_boxes)
        self.text, self.fps = rc.fused_module(elem, self.res, bounds, red, self.in_boxes, body)
        pointwise = body in ("sum", "dot", "div")
        share = all(tuple(map(tuple, b)) == tuple(map(tuple, self.res)) for b in self.in_boxes)
        assert rc.fused_path(self.dt, pointwise, res_shape, red[0], red[1], share) == path, (res_shape, red, body)
        self.path, self.div_zero, self.scale_exp = path, div_zero, scale_exp

    def __repr__(self):
        return f"{self.path}:{self.body}:{self.res[1]}:{self.red}"

    @property
    def ext(self):
        return tuple(h - l for l, h in zip(*self.red))

    def inputs(self, seed):
        """exact data: integers so small that every body value is exact and sum|body value| <= 2^p"""
        nin = len(self.in_boxes)
        n = max(1, int(np.prod(self.ext)))
        p = rc.P_BITS[np.dtype(self.dt)]
        if self.body == "dot":
            m = max(1, int(math.isqrt((1 << p) // (2 * n))))
        else:
            m = max(1, (1 << p) // (8 * n))
        m = min(m, 1 << 10)
        xs = []
        for k, (lb, ub) in enumerate(self.in_boxes):
            shape = tuple(u - l for l, u in zip(lb, ub))
            if self.body == "div" and k == 1:
                rng = np.random.default_rng(seed + k)
                x = rng.choice(np.array([1.0, -1.0, 0.5, -0.5]), size=shape).astype(self.dt)
            else:
                x = rc.exact_field(shape, self.dt, seed=seed + k, max_abs=m, bound_bits=p, scale_exp=self.scale_exp)
            xs.append(x)
        return xs

    def values(self, xs):
        """the oracle's per-cell values of the apply (copy-through outside apply.bounds), over the result box"""
        out = np.zeros(tuple(self.res[1]), self.dt)
        with np.errstate(all="ignore"):
            oracle.Module.parse(self.text).call("vals", out, *[x.copy() for x in xs])
        return out

    def red_slices(self):
        return tuple(slice(l, h) for l, h in zip(*self.red))

    def poison(self, xs):
        """NaN at every input cell a correct kernel never uses; div: input 1 is 0 on the copy-through cells"""
        masks = rc.fused_sentinel_masks(self.res, self.bounds, self.red, self.in_boxes, self.fps)
        ys = [x.copy() for x in xs]
        for y, m in zip(ys, masks):
            y[m] = NAN
        if self.div_zero:
            through = np.zeros(self.res[1], bool)
            through[self.red_slices()] = True
            through[tuple(slice(l, h) for l, h in zip(*self.bounds))] = False
            assert through.any()
            ys[1][through] = 0.0
            ys[0][tuple(slice(l, l + 1) for l in self.red[0])] = 0.0      # 0/0 on one copy-through cell
        return ys


def _B(shape):
    return ((1,) * len(shape), tuple(n - 1 for n in shape))


def _fused_exact_cases():
    cs = []
    for e in ("f64", "f32"):
        v = 2 if e == "f64" else 4
        cs += [
            # scalar kernel: stencil bodies, 1..3 inputs, inputs in boxes of their own (sh != 0), R across apply.bounds
            Fused(e, (4100,), _B((4100,)), ((0,), (4100,)), [], "stencil", "fused_scalar"),
            Fused(e, (33, 5000), _B((33, 5000)), ((0, 1), (33, 4998)), [((-1, -2), (35, 5003))], "stencil", "fused_scalar"),
            Fused(e, (9, 7, 300), _B((9, 7, 300)), ((0, 1, 1), (9, 7, 298)),
                  [((0, 0, -1), (9, 7, 302)), ((-1, 0, 0), (10, 7, 300))], "stencil", "fused_scalar"),
            Fused(e, (6, 5, 130), _B((6, 5, 130)), ((0, 0, 1), (6, 5, 129)), [((0, 0, 0), (6, 5, 130))], "dot", "fused_scalar"),
            Fused(e, (40, 260), _B((40, 260)), ((0, 0), (40, 260)), [((-3, -1), (42, 261))], "dot", "fused_scalar"),
            # dead slots and the 2048-workgroup cap: 8 * 2048 - 1 and 8 * 2048 + 1 one-chunk rows
            Fused(e, (16387, 260), _B((16387, 260)), ((1, 2), (16384, 258)), [], "stencil", "fused_scalar"),
            Fused(e, (16387, 260), _B((16387, 260)), ((1, 2), (16386, 258)), [], "stencil", "fused_scalar"),
            # vector kernel: pointwise bodies on aligned whole rows, 1..3 inputs, R across apply.bounds
            Fused(e, (70000,), _B((70000,)), ((0,), (70000,)), [], "dot", "fused_vec"),
            Fused(e, (33, 4096), _B((33, 4096)), ((0, 0), (32, 4096)), [((0, 0), (33, 4096))], "dot", "fused_vec"),
            Fused(e, (7, 9, 1100), _B((7, 9, 1100)), ((0, 0, 0), (6, 9, 1100)),
                  [((0, 0, 0), (7, 9, 1100))] * 2, "sum", "fused_vec"),
            Fused(e, (5, 3, 4 * 256 * v + 4 * v), _B((5, 3, 4 * 256 * v + 4 * v)),
                  ((1, 0, 2 * v), (5, 3, 4 * 256 * v + 3 * v)), [], "sum", "fused_vec"),
            # 4 * 2048 +- 1 chunks of 256 * VK cells: the cap, dead slots
            Fused(e, (4 * 2048 + 3, 256 * v), _B((4 * 2048 + 3, 256 * v)), ((1, 0), (4 * 2048, 256 * v)), [], "sum", "fused_vec"),
            Fused(e, (4 * 2048 + 3, 256 * v), _B((4 * 2048 + 3, 256 * v)), ((1, 0), (4 * 2048 + 2, 256 * v)), [], "sum", "fused_vec"),
            # a body that divides by input 1, which is 0 exactly on the copy-through cells: evaluated there, discarded
            Fused(e, (40, 1032), _B((40, 1032)), ((0, 0), (40, 1032)), [((0, 0), (40, 1032))], "div", "fused_vec", div_zero=True),
            Fused(e, (40, 1032), _B((40, 1032)), ((0, 1), (40, 1031)), [((0, 0), (40, 1032))], "div", "fused_scalar", div_zero=True),
            # subnormal data
            Fused(e, (33, 4096), _B((33, 4096)), ((0, 0), (32, 4096)), [], "sum", "fused_vec", scale_exp=-1074 if e == "f64" else -149),
            Fused(e, (9, 7, 300), _B((9, 7, 300)), ((0, 1, 1), (9, 7, 298)), [], "stencil", "fused_scalar",
                  scale_exp=-1074 if e == "f64" else -149),
        ]
    return cs


FUSED_EXACT = _fused_exact_cases()


@pytest.mark.parametrize("case", FUSED_EXACT, ids=repr)
def test_fused_reduce_is_exact_with_nan_at_every_unused_input_cell(nh, lower, case):
    xs = case.inputs(seed=int(np.prod(case.res[1])) % 9973)
    ys = case.poison(xs)
    vals = case.values(ys)
    x = vals[case.red_slices()]
    assert np.isfinite(x).all()
    assert rc.abs_sum_exact(x) <= 2 ** (rc.P_BITS[np.dtype(case.dt)] + case.scale_exp)
    want = rc.exact_sum(x)
    if case.scale_exp:
        assert want != 0 and (np.abs(x[x != 0]) < np.finfo(case.dt).tiny).all()
    mod = lower(case.text)
    assert [a["kernel"] for a in mod.report["applies"] if a["function"] == "red"] == ["reduce"]
    got = mod.call("red", *[nh.torch.from_numpy(y).cuda() for y in ys])
    assert _same(got, want, case.dt), (case, got, want)
    # the oracle's serial loop agrees on exact data
    with np.errstate(all="ignore"):
        assert _same(float(oracle.Module.parse(case.text).call("red", *[y.copy() for y in ys])), want, case.dt)


def _fused_special_cases():
    cs = []
    for e in ("f64", "f32"):
        cs += [Fused(e, (33, 4096), _B((33, 4096)), ((0, 0), (32, 4096)), [], "sum", "fused_vec"),
               Fused(e, (9, 7, 300), _B((9, 7, 300)), ((0, 1, 1), (9, 7, 298)), [], "sum", "fused_scalar"),
               Fused(e, (9, 7, 300), _B((9, 7, 300)), ((0, 1, 1), (9, 7, 298)), [], "stencil", "fused_scalar"),
               Fused(e, (9, 7, 300), _B((9, 7, 300)), ((0, 1, 1), (0, 7, 298)), [], "stencil", "fused_scalar")]
    return cs


FUSED_SPECIAL = _fused_special_cases()


@pytest.mark.parametrize("case", FUSED_SPECIAL, ids=repr)
def test_fused_reduce_special_values(nh, lower, case):
    mod = lower(case.text)
    torch = nh.torch
    red = lambda *ys: mod.call("red", *[torch.from_numpy(y).cuda() for y in ys])   # noqa: E731
    shape = case.res[1]
    if any(h <= l for l, h in zip(*case.red)):                   # empty reduced box: +0.0, no launch
        assert _bits(red(np.full(shape, NAN, case.dt)), case.dt) == 0
        return
    lo, hi = case.red
    first, last = tuple(lo), tuple(h - 1 for h in hi)
    inside = tuple(max(l, b) for l, b in zip(lo, case.bounds[0]))
    through = tuple(lo)                                           # plane 0 lies outside apply.bounds
    assert any(t < b for t, b in zip(through, case.bounds[0]))
    cells = {"first": first, "last": last, "copy-through": (0,) + tuple(hi_ - 2 for hi_ in hi[1:]), "inside": inside}
    if case.path == "fused_scalar":
        cells["row tail"] = inside[:-1] + (hi[-1] - 1,)          # the clamped last, partial chunk of a row
    for name, cell in cells.items():
        x = np.zeros(shape, case.dt)
        x[cell] = NAN
        assert math.isnan(red(x)), name
    # copy-through cells on plane 0: no cell of apply.bounds reads them, so each enters the sum exactly once
    x = np.zeros(shape, case.dt)
    x[through] = np.inf
    assert red(x) == math.inf
    x[cells["copy-through"]] = -np.inf
    assert math.isnan(red(x))
    if case.body == "sum":                                        # identity body: an inside cell enters once too
        x = np.zeros(shape, case.dt)
        x[inside] = np.inf
        assert red(x) == math.inf
        x[through] = -np.inf
        assert math.isnan(red(x))
    assert _bits(red(np.full(shape, -0.0, case.dt)), case.dt) == 0
    xs = [rc.exact_field(shape, case.dt, seed=2, scale_exp=-1074 if case.dt == F64 else -149, max_abs=16)]
    ys = case.poison(xs)
    want = rc.exact_sum(case.values(ys)[case.red_slices()])
    assert want != 0 and _same(red(*ys), want, case.dt)


# ---- general data against math.fsum: the tree-height bound ---------------------------------------------------------
def _cancelling(shape, dt, seed):
    """x and -x at scattered positions plus a few small values: a sum far below sum|x|"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = np.zeros(n, dt)
    pos = rng.permutation(n)
    h = n // 2
    big = helpers.hash_field((h,), dt, seed=seed) * dt(1000)
    x[pos[:h]] = big
    x[pos[h:2 * h]] = -big
    x[pos[:7]] += helpers.hash_field((7,), dt, seed=seed + 1) * dt(1e-3)
    return x.reshape(shape)


def _ratio(got, x, path, dt, ext):
    x64 = x.astype(np.float64).reshape(-1)
    ref = math.fsum(x64)
    bound = rc.gamma(rc.tree_height(path, dt, ext), dt) * math.fsum(np.abs(x64))
    return abs(got - ref) / bound if bound > 0 else 0.0


def _record(record_testsuite_property, path, dt, r):
    """the ratio is part of the report (a property of the junit-xml test suite, and a line of output under -s)"""
    record_testsuite_property(f"gamma_ratio {path} {np.dtype(dt).name}", f"{r:.3e}")
    print(f"gamma-ratio {path} {np.dtype(dt).name} {r:.3e}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("path", ["flat", "box"])
def test_plain_reduce_within_the_tree_height_bound(nh, record_testsuite_property, dt, path):
    for shape, box in rc.GAMMA_PLAIN[path]:
        assert rc.plain_path(shape, box) == path
        ext = rc.box_ext(shape, box)
        sl = rc.box_slices(box, len(shape))
        for x in (helpers.hash_field(shape, dt, seed=41), _cancelling(shape, dt, seed=42)):
            got = _plain_sum(nh, x, box)
            r = _ratio(got, x[sl], path, dt, ext)
            _record(record_testsuite_property, path, dt, r)
            assert r <= 1.0, (shape, box, got, r)


def _fused_gamma_cases():
    cs = []
    for e in ("f64", "f32"):
        for path, body in (("fused_scalar", "stencil"), ("fused_vec", "dot")):
            for shape, red in rc.GAMMA_FUSED[path]:
                nin = 2 if body == "dot" else 1
                cs.append(Fused(e, shape, _B(shape), red, [((0,) * len(shape), shape)] * (nin - 1), body, path))
    return cs


FUSED_GAMMA = _fused_gamma_cases()


@pytest.mark.parametrize("case", FUSED_GAMMA, ids=repr)
def test_fused_reduce_within_the_tree_height_bound(nh, lower, record_testsuite_property, case):
    """x is the oracle's apply value per cell (bit-identical to the device's, tests/test_scalar_ops_gpu.py), so only the
    summation is bounded"""
    mod = lower(case.text)
    shape = case.res[1]
    nin = len(case.in_boxes)
    for xs in ([helpers.hash_field(shape, case.dt, seed=50 + k) for k in range(nin)],
               [_cancelling(shape, case.dt, seed=60)] + [np.ones(shape, case.dt)] * (nin - 1)):
        got = mod.call("red", *[nh.torch.from_numpy(x).cuda() for x in xs])
        x = case.values(xs)[case.red_slices()]
        r = _ratio(got, x, case.path, case.dt, case.ext)
        _record(record_testsuite_property, case.path, case.dt, r)
        assert r <= 1.0, (case, got, r)


# ---- beyond 2^31 cells ----------------------------------------------------------------------------------------------
def _sparse_pm1_(torch, t, gen, density_log2=9):
    """fill t in place, slab by slab along dim 0, with +-1 at about 2 / 2^density_log2 of the cells, 0 elsewhere"""
    for s in range(0, t.shape[0], max(1, t.shape[0] // 64)):
        sl = t[s:s + max(1, t.shape[0] // 64)]
        r = torch.randint(0, 1 << density_log2, sl.shape, device="cuda", dtype=torch.int16, generator=gen)
        sl.copy_((r == 0).to(t.dtype) - (r == 1).to(t.dtype))
        del r


def _int_sum(torch, t, f=None):
    """exact sum in int64 on the device, one slab along dim 0 at a time; f(slab, start, rows) maps a slab first"""
    tot = 0
    step = max(1, t.shape[0] // 64)
    for s in range(0, t.shape[0], step):
        a = t[s:s + step]
        if f is not None:
            a = f(a, s, step)
        tot += int(a.to(torch.int64).sum().item())
    return tot


def _abs(t, s, n):
    return t.abs()


PEAK_BYTES = 19 * 10 ** 9   # the big fields and every slab temporary, below about 20 GB of device memory


def test_flat_reduce_beyond_2_pow_31_cells(nh):
    torch = nh.torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    n = 2 ** 31 + 2 ** 20 + 3                           # f32: 8.6 GB, n % 4 != 0: a scalar tail
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    x = torch.empty((n,), dtype=torch.float32, device="cuda")
    f = None
    try:
        _sparse_pm1_(torch, x.view(-1)[: n - 3].view(64, -1), gen)
        x[n - 3:] = torch.tensor([1.0, -1.0, 1.0], device="cuda")
        x[0] = 1.0
        want = _int_sum(torch, x[: n - 3].view(64, -1)) + 1
        assert 0 < abs(want) < 2 ** 24 and _int_sum(torch, x[: n - 3].view(64, -1), _abs) < 2 ** 24
        f = nh.fields.DeviceField((0,), (n,), nh.capi.F32, tensor=x)
        assert rc.plain_path((n,), None) == "flat"
        got = nh.apply.reduce_sum(f)
        assert got == float(want), (got, want)
        x[n - 1] = float("nan")                         # the last cell lies in the tail
        assert math.isnan(nh.apply.reduce_sum(f))
        assert torch.cuda.max_memory_allocated() < PEAK_BYTES
    finally:
        del x, f
        torch.cuda.empty_cache()


FUSED_HUGE = [Fused("f32", (1100, 1000, 2000), ((0, 0, 0), (1100, 1000, 2000)), ((0, 0, 0), (1100, 1000, 2000)),
                    [((0, 0, 0), (1100, 1000, 2000))], "dot", "fused_vec"),
              Fused("f32", (1100, 1000, 2000), ((0, 0, 0), (1100, 1000, 2000)), ((0, 0, 1), (1100, 1000, 2000)),
                    [((0, 0, 0), (1100, 1000, 2000))], "dot", "fused_scalar")]


def test_fused_dot_product_beyond_2_pow_31_cells(nh, lower):
    """a rank-3 dot product of 2.2e9 cells (rows and row count inside the host's 31-bit limit), on both fused kernels;
    two f32 fields of 8.8 GB"""
    torch = nh.torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    shape = (1100, 1000, 2000)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    a = torch.empty(shape, dtype=torch.float32, device="cuda")
    b = torch.empty(shape, dtype=torch.float32, device="cuda")
    try:
        _sparse_pm1_(torch, a, gen)
        step = max(1, shape[0] // 64)
        for s in range(0, shape[0], step):               # dense random signs
            r = torch.randint(0, 2, b[s:s + step].shape, device="cuda", dtype=torch.int8, generator=gen)
            b[s:s + step].copy_(r.to(torch.float32) * 2 - 1)
            del r
        a[-1, -1, -1], b[-1, -1, -1] = 1.0, 1.0
        a[0, 0, 0], b[0, 0, 0] = 1.0, -1.0
        want_vec = _int_sum(torch, a, lambda t, s, n: t * b[s:s + n])
        want_scalar = want_vec - _int_sum(torch, a[:, :, 0], lambda t, s, n: t * b[s:s + n, :, 0])
        assert _int_sum(torch, a, _abs) < 2 ** 24
        for case, want in zip(FUSED_HUGE, (want_vec, want_scalar)):
            got = lower(case.text).call("red", a, b)
            assert got == float(want), (case, got, want)
        assert torch.cuda.max_memory_allocated() < PEAK_BYTES
    finally:
        del a, b
        torch.cuda.empty_cache()
