"""Monitored applies on the GPU: a monitored launch returns the plain launch's result bit for bit and, out of
the same launch, S = sum (new - old)^2 over apply.bounds x launch region, on every launch form that has a monitored path.

Shapes are the smallest that still cross chunk seams, partial tiles and a tail launch.  For every case and configuration:
 1. `out` (sentinel-filled first) equals the plain __geom launch and the oracle bit for bit;
 2. S agrees with the sum of the terms computed from the oracle's fields in numpy -- (new - old), then squared, in T, summed
    with math.fsum -- within 2 (n - 1) eps sum |x_i|, the bound tests/test_reduce_gpu.py states for any two summation orders
    (the terms themselves are identical on both sides);
 3. two runs of one configuration give the same bits of S;
 4. with input 0 holding +inf at every cell outside apply.bounds S is still finite and within the bound (a kernel that
    counted a copy-through or clamped cell would produce inf - inf = NaN); zero-trip bounds give exactly +0.
    A stencil that reads input 0's neighbours carries that +inf INTO the cells next to the boundary whatever the kernel
    does, so this check runs on the two-input form of each case -- the neighbours come from a second field, input 0 is read
    at the centre only (monitor_cases.star_module halo_on_second) -- on the same shapes and configurations;
 5. sum_out inside a field is NEPTUNE_HIP_EINVAL and nothing is written."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import monitor_cases as mc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

SENTINEL = -777.25

# name: (shape, dtype, origin, bounds or None = one cell inside on every side)
CASES = {
    "r3_f64_20x37x130": ((20, 37, 130), np.float64, None, None),
    "r3_f64_9x21x133_ragged": ((9, 21, 133), np.float64, None, None),
    "r3_f32_11x19x260_origin": ((11, 19, 260), np.float32, (3, -2, 5), None),
    "r2_f64_70x264": ((70, 264), np.float64, None, None),
    "r2_f32_35x133": ((35, 133), np.float32, None, None),
    "r1_f64_1000": ((1000,), np.float64, None, None),
    "r3_f64_zero_trip": ((9, 21, 133), np.float64, None, ([4, 1, 1], [4, 20, 132])),
}


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import os
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache"))
    from neptune_hip import _capi, apply, fields, lowering

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering = torch, _capi, apply, fields, lowering
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    return ns


def _configs(nh, rank):
    """(name, cfg, region0): the automatic plan, every march tile the module holds with chunks of 1 and 3 planes, both direct
    forms, and a launch region restricted along dim 0 on the automatic plan and on the direct kernel"""
    cf, K = nh.apply.make_cfg, nh.capi
    out = [("auto", None, None), ("rows", cf(K.KERNEL_DIRECT), None), ("flat", cf(K.KERNEL_DIRECT, flags=K.FLAG_DIRECT_FLAT), None)]
    for v in range({3: 8, 2: 3, 1: 1}[rank]):
        for chunk in (1, 3):
            out.append((f"tile{v}_chunk{chunk}", cf(K.KERNEL_MARCH, v, chunk), None))
    if rank > 1:
        out += [("auto_region", None, True), ("rows_region", cf(K.KERNEL_DIRECT), True)]
    return out


def _run_case(nh, name, two_input):
    shape, dtype, origin, bounds = CASES[name]
    rank = len(shape)
    origin = [0] * rank if origin is None else list(origin)
    if bounds is None:
        bounds = ([o + 1 for o in origin], [o + n - 1 for o, n in zip(origin, shape)])
    text = mc.star_module(shape, dtype, origin, bounds, halo_on_second=two_input)
    mod = nh.lowering.compile_module(text, norm_entries=True)
    entry = mod.norm_entry("entry")
    assert entry.fn_norm is not None and entry.symbol == "entry_0__geom"
    u = helpers.hash_field(shape, dtype, seed=41)
    v = helpers.hash_field(shape, dtype, seed=42)
    everywhere = mc.inside_slices(shape, origin, bounds)
    if two_input:   # check 4: +inf in input 0 at every cell outside apply.bounds
        mask = np.ones(shape, bool)
        mask[everywhere] = False
        u = u.copy()
        u[mask] = np.inf
    want = np.zeros_like(u)
    args = (want, u, v) if two_input else (want, u)
    with np.errstate(invalid="ignore"):
        helpers.oracle.Module.parse(text).call("entry", *args)
    F = nh.fields.DeviceField
    ins = [F.from_numpy(u, lb=origin)] + ([F.from_numpy(v, lb=origin)] if two_input else [])
    empty = any(lo >= hi for lo, hi in zip(*bounds))
    ran = 0
    for cname, cfg, region in _configs(nh, rank):
        region0 = (2, shape[0] - 3) if region else None
        reg = None if region0 is None else ([region0[0]] + [0] * (rank - 1), [region0[1]] + list(shape[1:]))
        where = mc.inside_slices(shape, origin, bounds, region0)
        ref, bound = mc.reference_sum(want, u, where)
        assert math.isfinite(ref)
        outs, sums = [], []
        for rep in range(2):
            out = F.empty_like(ins[0])
            out.tensor.fill_(SENTINEL)
            s = nh.apply.apply_norm(entry, ins, out, bounds, region=reg, cfg=cfg)
            outs.append(out)
            sums.append(s)
        what = f"{name} two_input={two_input} {cname}"
        if sums[0] is None:
            # no monitored form for this request (a tile that stands for the plane-in-LDS kernel): nothing was launched
            assert cfg is not None and cfg.kernel == nh.capi.KERNEL_MARCH, what
            assert bool((outs[0].tensor == SENTINEL).all()), what
            continue
        ran += 1
        plain = F.empty_like(ins[0])
        plain.tensor.fill_(SENTINEL)
        nh.apply.apply_builtin(entry, ins, plain, bounds, region=reg, cfg=cfg)
        nh.torch.cuda.synchronize()
        got = outs[0].numpy()
        expect = want
        if region0 is not None:   # outside the launch region nothing is stored
            expect = np.full_like(want, SENTINEL)
            expect[region0[0]:region0[1]] = want[region0[0]:region0[1]]
        assert bits_equal(got, plain.numpy()), what + "\n" + mismatch_report(got, plain.numpy())      # 1
        assert bits_equal(got, expect), what + "\n" + mismatch_report(got, expect)
        s = sums[0]
        print(f"{what}: S = {s!r} reference = {ref!r} |diff| = {abs(s - ref):.3e} bound = {bound:.3e}")
        assert math.isfinite(s) and abs(s - ref) <= bound, what                                      # 2, 4
        assert np.float64(sums[0]).tobytes() == np.float64(sums[1]).tobytes(), what                  # 3
        if empty:
            assert s == 0.0 and math.copysign(1.0, s) == 1.0, what                                   # exactly +0
    assert ran >= 3
    return entry, ins, bounds


@pytest.mark.parametrize("name", list(CASES))
def test_monitored_launch_matches_plain_launch_and_reference_sum(nh, name):
    entry, ins, bounds = _run_case(nh, name, two_input=False)
    # 5: sum_out inside a field is refused and nothing is written
    F = nh.fields.DeviceField
    out = F.empty_like(ins[0])
    out.tensor.fill_(SENTINEL)
    before = ins[0].numpy().copy()
    g = nh.apply.geom_for(ins, out, bounds)
    arr = (C.c_void_p * len(ins))(*[f.ptr for f in ins])
    elem = out.tensor.element_size()
    for target in (out.ptr + 3 * elem, ins[0].ptr + 5 * elem):
        rc = entry.fn_norm(C.byref(g), arr, out.ptr, target, nh.fields.current_stream_ptr(), None)
        assert rc == nh.capi.EINVAL
    nh.torch.cuda.synchronize()
    assert bool((out.tensor == SENTINEL).all()) and bits_equal(ins[0].numpy(), before)


@pytest.mark.parametrize("name", list(CASES))
def test_cells_outside_the_bounds_never_count(nh, name):
    _run_case(nh, name, two_input=True)


@pytest.mark.parametrize("body,kind,shape", [("BODY_LAP3D7_F64", "3d7", (20, 37, 130)), ("BODY_LAP2D5_F64", "2d5", (70, 264))])
def test_builtin_bodies_through_the_c_abi(nh, body, kind, shape):
    body_id = getattr(nh.capi, body)
    u = helpers.hash_field(shape, np.float64, seed=43)
    want = helpers.oracle_entry(kind, u)
    bounds = ([1] * len(shape), [n - 1 for n in shape])
    ref, bound = mc.reference_sum(want, u, mc.inside_slices(shape, [0] * len(shape), bounds))
    F = nh.fields.DeviceField
    fin = F.from_numpy(u)
    cf, K = nh.apply.make_cfg, nh.capi
    ntiles = nh.lib.neptune_hip_march_variant_count(len(shape))
    cfgs = [None, cf(K.KERNEL_DIRECT), cf(K.KERNEL_DIRECT, flags=K.FLAG_DIRECT_FLAT)] + \
           [cf(K.KERNEL_MARCH, v, 3) for v in sorted({0, 1, 3, 6, ntiles - 1})]
    ran = 0
    for cfg in cfgs:
        out = F.empty_like(fin)
        out.tensor.fill_(SENTINEL)
        s = nh.apply.apply_norm(body_id, [fin], out, bounds, cfg=cfg)
        if s is None:
            assert bool((out.tensor == SENTINEL).all())
            continue
        ran += 1
        assert bits_equal(out.numpy(), want), mismatch_report(out.numpy(), want)
        assert abs(s - ref) <= bound
        assert s == nh.apply.apply_norm(body_id, [fin], out, bounds, cfg=cfg)
    assert ran >= 5
    # the device scalar of the asynchronous form, and the refusals of neptune_hip_apply_builtin
    dst = nh.torch.zeros(1, dtype=nh.torch.float64, device="cuda")
    out = F.empty_like(fin)
    assert nh.apply.apply_norm(body_id, [fin], out, bounds, sum_out=dst) is dst
    nh.torch.cuda.synchronize()
    assert abs(float(dst.item()) - ref) <= bound
    g = nh.apply.geom_for([fin], out, bounds)
    arr = (C.c_void_p * 1)(fin.ptr)
    st = nh.fields.current_stream_ptr()
    assert nh.lib.neptune_hip_apply_builtin_norm(body_id, C.byref(g), arr, out.ptr, out.ptr + 8, st, None) == K.EINVAL
    assert nh.lib.neptune_hip_apply_builtin_norm(body_id, C.byref(g), arr, fin.ptr, dst.data_ptr(), st, None) == K.EINVAL
    assert nh.lib.neptune_hip_apply_builtin_norm(99, C.byref(g), arr, out.ptr, dst.data_ptr(), st, None) == K.EINVAL


_DIFFSQ = """
#l = #neptune_ir.location<"cell">
#b = #neptune_ir.bounds<lb = [0, 0, 0], ub = [{ub}]>
!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>
!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>
module {{
  func.func @diffsq(%a: memref<?x?x?x{elem}>, %b: memref<?x?x?x{elem}>) -> {elem} {{
    %fa = neptune_ir.wrap %a : memref<?x?x?x{elem}> -> !f
    %fb = neptune_ir.wrap %b : memref<?x?x?x{elem}> -> !f
    %u = neptune_ir.load %fa : !f -> !t
    %v = neptune_ir.load %fb : !f -> !t
    %sq = neptune_ir.apply(%u, %v) attributes {{bounds = #b}} : (!t, !t) -> !t {{
      ^bb0(%i: index, %j: index, %k: index, %x: !t, %y: !t):
        %p = neptune_ir.access %x[0, 0, 0] : !t -> {elem}
        %q = neptune_ir.access %y[0, 0, 0] : !t -> {elem}
        %d = arith.subf %p, %q : {elem}
        %e = arith.mulf %d, %d : {elem}
        neptune_ir.yield %e : {elem}
    }}
    %s = neptune_ir.reduce %sq in #b {{kind = "sum"}} : !t -> {elem}
    func.return %s : {elem}
  }}
}}
"""


@pytest.mark.parametrize("shape,dtype", [((5, 7, 520), np.float64), ((5, 7, 519), np.float64),
                                         ((3, 9, 1028), np.float32), ((3, 9, 1027), np.float32)])
def test_update_norm_returns_the_bits_of_the_lowered_fused_reduce(nh, shape, dtype):
    """neptune_hip_update_norm(a, b) and a lowered reduce(apply((a - b) * (a - b))) over the whole box run the same kernels
    on one launch plan (plan_reduce_apply, csrc/kernels/reduce_launch.hpp), so on the same device buffers they return the
    same bits: no tolerance.  The first shape of each pair takes the vector kernel with two chunks per row, the second the
    scalar kernel with a ragged last chunk."""
    elem = "f64" if dtype == np.float64 else "f32"
    tdtype = nh.torch.float64 if dtype == np.float64 else nh.torch.float32
    F = nh.fields.DeviceField
    a = F.from_numpy(helpers.hash_field(shape, dtype, seed=51))
    b = F.from_numpy(helpers.hash_field(shape, dtype, seed=52))
    mod = nh.lowering.compile_module(_DIFFSQ.format(ub=", ".join(map(str, shape)), elem=elem))
    assert [x["kernel"] for x in mod.report["applies"]] == ["reduce"]
    lowered = mod.call("diffsq", a.tensor, b.tensor)
    dst = nh.torch.full((1,), -1.0, dtype=tdtype, device="cuda")
    g = nh.apply.geom_for([b], a, ([0, 0, 0], list(shape)))
    cdtype = nh.capi.F64 if dtype == np.float64 else nh.capi.F32
    nh.capi.check(nh.lib.neptune_hip_update_norm(cdtype, C.byref(g), a.ptr, b.ptr, dst.data_ptr(), nh.fields.current_stream_ptr()),
                  "update_norm")
    nh.torch.cuda.synchronize()
    direct = float(dst.item())
    print(f"{shape} {elem}: update_norm = {direct!r} lowered = {lowered!r}")
    assert math.isfinite(direct) and direct > 0.0
    assert np.float64(direct).tobytes() == np.float64(lowered).tobytes()
