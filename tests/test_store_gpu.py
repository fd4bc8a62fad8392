"""neptune_store_box (csrc/kernels/util_kernels.hpp), the kernel behind every bounded neptune_ir.store, on its own: against
NumPy slicing, bit for bit, with the destination pre-filled with a sentinel that every cell outside the box must keep.

Rows of 256 VK - 1, 256 VK, 256 VK + 1 and 2 * 256 VK + 3 cells (VK cells per 16-byte word: one workgroup moves 256 VK cells
of a row, so these end a row one cell short of a chunk, on it, one cell into the next and three cells into the third),
row starts at every cell offset within a 16-byte word in the source and, independently, in the destination, on fields
whose rows are whole words long and on ragged ones (every row at another offset), leading extents 1 and 3, boxes one cell
thick or empty along each axis -- and run_store's loop over the leading indices of a rank-4 and a rank-5 field, through a
lowered module whose only work is such a store."""
import os

import numpy as np
import pytest

import helpers
from helpers import bits_equal, mismatch_report, oracle

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
VK = {np.float64: 2, np.float32: 4}


@pytest.fixture(scope="module")
def nh(built_libs):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from neptune_hip import _capi, apply, fields
    lib = _capi.load()
    lib.neptune_hip_init(0)

    class NS:
        pass
    ns = NS()
    ns.capi, ns.apply, ns.fields, ns.lib, ns.torch = _capi, apply, fields, lib, torch
    return ns


def _store_and_check(nh, fs, s, dst_lb, dst_shape, lb, ub):
    """store box [lb, ub) of the device field fs (host copy s) into a fresh sentinel-filled field; compare with slicing"""
    fd = nh.fields.DeviceField(dst_lb, [l + n for l, n in zip(dst_lb, dst_shape)], fs.dtype)
    fd.tensor.fill_(SENTINEL)
    nh.apply.store(fs, fd, (list(lb), list(ub)))
    nh.torch.cuda.synchronize()
    want = np.full(dst_shape, SENTINEL, s.dtype)
    if all(u > l for l, u in zip(lb, ub)):
        want[tuple(slice(l - o, u - o) for l, u, o in zip(lb, ub, dst_lb))] = s[tuple(slice(l - o, u - o) for l, u, o in zip(lb, ub, fs.lb))]
    got = fd.numpy()
    assert bits_equal(got, want), f"src {fs.lb} {fs.shape} dst {dst_lb} {dst_shape} box {lb} {ub}\n" + mismatch_report(got, want)
    return want


def _up(n, m):
    return (n + m - 1) // m * m


@pytest.mark.parametrize("rank", [1, 2, 3])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_long_rows_at_every_word_offset(nh, dt, rank):
    vk = VK[dt]
    lengths = [256 * vk - 1, 256 * vk, 256 * vk + 1, 2 * 256 * vk + 3]
    for lead in ((1, 3) if rank > 1 else (1,)):
        for ragged in (0, 1):
            # the source: two spare leading indices, and rows of whole words (ragged: one cell more, so that every row
            # starts at another offset within its word)
            src_lb = [2, -1, -3][3 - rank:]
            src_shape = [lead + 2] * (rank - 1) + [_up(max(lengths) + 3 * vk, vk) + ragged]
            s = helpers.hash_field(src_shape, dt, seed=17 + rank)
            fs = nh.fields.DeviceField.from_numpy(s, src_lb)
            moved = 0
            for n in lengths:
                for so in range(vk):
                    for do in range(vk):
                        lb = [l + 1 for l in src_lb[:-1]] + [src_lb[-1] + vk + so]        # physical column vk + so
                        ub = [l + lead for l in lb[:-1]] + [lb[-1] + n]
                        dst_lb = [l - 2 for l in lb[:-1]] + [lb[-1] - vk - do]           # physical column vk + do
                        dst_shape = [lead + 3] * (rank - 1) + [_up(n + 3 * vk, vk) + ragged]
                        want = _store_and_check(nh, fs, s, dst_lb, dst_shape, lb, ub)
                        moved += int((want != SENTINEL).sum())
            assert moved == vk * vk * sum(lengths) * lead ** (rank - 1)      # the field holds no sentinel: all cells arrived


@pytest.mark.parametrize("rank", [1, 2, 3])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_thin_and_empty_boxes_along_each_axis(nh, dt, rank):
    vk = VK[dt]
    src_lb = [-2, 3, -5][3 - rank:]
    src_shape = [6, 5, 256 * vk + 9][3 - rank:]
    dst_lb = [-3, 1, -6][3 - rank:]
    dst_shape = [8, 9, 256 * vk + 14][3 - rank:]
    s = helpers.hash_field(src_shape, dt, seed=29 + rank)
    fs = nh.fields.DeviceField.from_numpy(s, src_lb)
    lb0 = [l + 1 for l in src_lb]
    ub0 = [l + n - 1 for l, n in zip(src_lb, src_shape)]
    _store_and_check(nh, fs, s, dst_lb, dst_shape, lb0, ub0)
    for axis in range(rank):
        for at in (lb0[axis], (lb0[axis] + ub0[axis]) // 2, ub0[axis] - 1):
            lb, ub = list(lb0), list(ub0)
            lb[axis], ub[axis] = at, at + 1                                 # one cell thick
            want = _store_and_check(nh, fs, s, dst_lb, dst_shape, lb, ub)
            assert int((want != SENTINEL).sum()) == int(np.prod([u - l for l, u in zip(lb, ub)]))
            ub[axis] = at                                                   # empty
            want = _store_and_check(nh, fs, s, dst_lb, dst_shape, lb, ub)
            assert (want == SENTINEL).all()


# ---- rank 4 and 5: run_store copies one rank-3 box per leading index of the stored box --------------------------------
def _bnd(lb, ub):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, lb))}], ub = [{', '.join(map(str, ub))}]>"


def lead_store_module(elem, a, b, box):
    """@copy(a, b) -> b: store (load fa) to fb {bounds = box}; a, b, box: (lb, ub)"""
    mr = "x".join("?" * len(a[0])) + "x" + elem
    return f"""#l = #neptune_ir.location<"cell">
!ta = !neptune_ir.temp<element = {elem}, bounds = {_bnd(*a)}, location = #l>
!fa = !neptune_ir.field<element = {elem}, bounds = {_bnd(*a)}, location = #l>
!fb = !neptune_ir.field<element = {elem}, bounds = {_bnd(*b)}, location = #l>
module {{
  func.func @copy(%a: memref<{mr}>, %b: memref<{mr}>) -> memref<{mr}> {{
    %fa = neptune_ir.wrap %a : memref<{mr}> -> !fa
    %fb = neptune_ir.wrap %b : memref<{mr}> -> !fb
    %t = neptune_ir.load %fa : !fa -> !ta
    neptune_ir.store %t to %fb {{bounds = {_bnd(*box)}}} : !ta to !fb
    %r = neptune_ir.unwrap %fb : !fb -> memref<{mr}>
    func.return %r : memref<{mr}>
  }}
}}
"""


# element type, box of a, box of b (another origin along every axis), the stored box: a strict sub-box of both along the
# leading dimensions too, rows longer than one chunk of 256 VK cells
LEAD_CASES = {
    4: ("f64", ((1, -2, 3, -1), (5, 3, 9, 529)), ((0, -3, 1, -4), (6, 5, 9, 536)), ((2, -1, 4, 2), (4, 2, 8, 520))),
    5: ("f32", ((0, 1, -2, 3, -1), (4, 5, 3, 8, 1029)), ((-1, 0, -3, 1, -4), (4, 5, 4, 9, 1036)), ((1, 2, -1, 4, 1), (3, 4, 2, 7, 1028))),
}


@pytest.fixture(scope="module")
def lead_modules(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache_store"))
    from neptune_hip import lowering
    texts = {rank: lead_store_module(*case) for rank, case in LEAD_CASES.items()}
    helpers.prefetch_modules(list(texts.values()))
    return lowering, torch, texts


@pytest.mark.parametrize("rank", sorted(LEAD_CASES))
def test_bounded_store_per_leading_index(lead_modules, rank):
    lowering, torch, texts = lead_modules
    elem, a, b, box = LEAD_CASES[rank]
    dt = np.float64 if elem == "f64" else np.float32
    for (lb, ub) in (a, b):                                                 # strictly inside both, leading axes included
        assert all(l < p and q < u for l, u, p, q in zip(lb, ub, box[0], box[1]))
    shape_a, shape_b = (tuple(u - l for l, u in zip(*x)) for x in (a, b))
    ha = helpers.hash_field(shape_a, dt, seed=51 + rank)
    want = np.full(shape_b, SENTINEL, dt)
    assert oracle.Module.parse(texts[rank]).call("copy", ha.copy(), want) is want
    inside = np.zeros(shape_b, bool)
    inside[tuple(slice(p - l, q - l) for p, q, l in zip(box[0], box[1], b[0]))] = True
    assert (want[~inside] == SENTINEL).all() and not (want[inside] == SENTINEL).any()
    mod = lowering.compile_module(texts[rank])
    assert mod.report["lowered"] == ["copy"]
    for device in (True, False):
        ga = torch.from_numpy(ha.copy()).cuda() if device else ha.copy()
        gb = torch.full(shape_b, SENTINEL, dtype=ga.dtype, device="cuda") if device else np.full(shape_b, SENTINEL, dt)
        assert mod.call("copy", ga, gb) is gb
        got_a, got_b = (x.cpu().numpy() if device else x for x in (ga, gb))
        assert bits_equal(got_b, want), f"rank {rank} device={device}\n" + mismatch_report(got_b, want)
        assert bits_equal(got_a, ha)
