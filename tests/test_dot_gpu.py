"""Dot-monitored applies on the GPU: a dot-monitored launch returns the plain launch's result bit for bit and,
out of the same launch, D = sum new * old over apply.bounds x launch region (old = input 0 at the same physical index), on
every launch form that has a monitored path; neptune_hip_dot returns the same D from the two fields in one read-only pass.

Shapes are the smallest that still cross chunk seams, partial tiles and a tail launch (those of tests/test_monitor_gpu.py).
For every case and configuration:
 1. `out` (sentinel-filled first) equals the plain __geom launch and the oracle bit for bit;
 2. D agrees with the sum of the terms formed from the oracle's fields in numpy -- new * old, one rounding in T, summed with
    math.fsum -- within 2 (n - 1) eps sum |t_i|, what any two summation orders of the same terms may differ by;
 3. two runs of one configuration give the same bits of D;
 4. with a NaN in input 0 at every cell outside Omega, D is still finite and within the bound (a kernel that counted a
    copy-through or clamped cell would return NaN); zero-trip bounds give exactly +0.  As in the monitor tests this runs on the
    two-input form (neighbours from a second field), where input 0's values outside the bounds reach no cell inside;
 5. neptune_hip_dot(out, input 0) is within the same bound;
 6. dot_out inside a field is NEPTUNE_HIP_EINVAL, a plan onto the plane-in-LDS kernel NEPTUNE_HIP_EUNSUPPORTED, and neither
    writes anything."""
import ctypes as C
import math

import numpy as np
import pytest

import cg_cases as cc
import helpers
import monitor_cases as mc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

SENTINEL = -777.25

# name: (shape, dtype, origin, bounds or None = one cell inside on every side)
CASES = {
    "r3_f64_20x37x130": ((20, 37, 130), np.float64, None, None),
    "r3_f64_9x11x131_ragged": ((9, 11, 131), np.float64, None, None),
    "r3_f32_11x19x260_origin": ((11, 19, 260), np.float32, (3, -2, 5), None),
    "r2_f64_70x264": ((70, 264), np.float64, None, None),
    "r2_f32_35x131": ((35, 131), np.float32, None, None),
    "r1_f64_1000": ((1000,), np.float64, None, None),
    "r3_f64_zero_trip": ((9, 11, 131), np.float64, None, ([4, 1, 1], [4, 10, 130])),
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
    text = mc.star_module(shape, dtype, origin, bounds, centre=float(4 * rank), side=-1.0, halo_on_second=two_input)
    mod = nh.lowering.compile_module(text, dot_entries=True)
    entry = mod.dot_entry("entry")
    assert entry.fn_dot is not None and entry.fn_norm is None and entry.symbol == "entry_0__geom"
    u = helpers.hash_field(shape, dtype, seed=61)
    v = helpers.hash_field(shape, dtype, seed=62)
    everywhere = mc.inside_slices(shape, origin, bounds)
    if two_input:   # check 4: NaN in input 0 at every cell outside apply.bounds
        mask = np.ones(shape, bool)
        mask[everywhere] = False
        u = u.copy()
        u[mask] = np.nan
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
        ref, bound = cc.dot_terms(want, u, where)
        assert math.isfinite(ref)
        outs, dots = [], []
        for rep in range(2):
            out = F.empty_like(ins[0])
            out.tensor.fill_(SENTINEL)
            outs.append(out)
            dots.append(nh.apply.apply_dot(entry, ins, out, bounds, region=reg, cfg=cfg))
        what = f"{name} two_input={two_input} {cname}"
        if dots[0] is None:
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
        d = dots[0]
        two = nh.apply.dot(outs[0], ins[0], bounds, region=reg)
        print(f"{what}: D = {d!r} reference = {ref!r} |diff| = {abs(d - ref):.3e} two-field = {two!r} bound = {bound:.3e}")
        assert math.isfinite(d) and abs(d - ref) <= bound, what                                       # 2, 4
        assert np.float64(dots[0]).tobytes() == np.float64(dots[1]).tobytes(), what                   # 3
        assert math.isfinite(two) and abs(two - ref) <= bound, what                                   # 5
        if empty:
            assert d == 0.0 and math.copysign(1.0, d) == 1.0 and two == 0.0 and math.copysign(1.0, two) == 1.0, what
    assert ran >= 3
    return entry, ins, bounds


@pytest.mark.parametrize("name", list(CASES))
def test_dot_monitored_launch_matches_plain_launch_and_reference_dot(nh, name):
    entry, ins, bounds = _run_case(nh, name, two_input=False)
    # 6: dot_out inside a field is refused and nothing is written
    F = nh.fields.DeviceField
    out = F.empty_like(ins[0])
    out.tensor.fill_(SENTINEL)
    before = ins[0].numpy().copy()
    g = nh.apply.geom_for(ins, out, bounds)
    arr = (C.c_void_p * len(ins))(*[f.ptr for f in ins])
    elem = out.tensor.element_size()
    for target in (out.ptr + 3 * elem, ins[0].ptr + 5 * elem):
        assert entry.fn_dot(C.byref(g), arr, out.ptr, target, nh.fields.current_stream_ptr(), None) == nh.capi.EINVAL
    nh.torch.cuda.synchronize()
    assert bool((out.tensor == SENTINEL).all()) and bits_equal(ins[0].numpy(), before)


@pytest.mark.parametrize("name", list(CASES))
def test_cells_outside_omega_never_count(nh, name):
    _run_case(nh, name, two_input=True)


def test_plane_in_lds_plan_is_refused(nh):
    """a radius-2 star held to the plane-in-LDS kernel by its tile, as tests/test_until_loop_gpu.py does"""
    shape = (12, 20, 136)
    mod = nh.lowering.compile_module(cc.cg_module(shape, radius=2), dot_entries=True)
    entry = mod.dot_entry("entry")
    F = nh.fields.DeviceField
    u = F.from_numpy(helpers.hash_field(shape, np.float64, seed=63))
    out = F.empty_like(u)
    out.tensor.fill_(SENTINEL)
    cfg = nh.apply.make_cfg(nh.capi.KERNEL_MARCH, 7)
    g = nh.apply.geom_for([u], out, cc.interior(shape, 2))
    dst = nh.torch.full((1,), 5.0, dtype=nh.torch.float64, device="cuda")
    rc = entry.fn_dot(C.byref(g), (C.c_void_p * 1)(u.ptr), out.ptr, dst.data_ptr(), nh.fields.current_stream_ptr(), C.byref(cfg))
    assert rc == nh.capi.EUNSUPPORTED
    assert nh.apply.apply_dot(entry, [u], out, cc.interior(shape, 2), cfg=cfg) is None
    nh.torch.cuda.synchronize()
    assert bool((out.tensor == SENTINEL).all()) and float(dst.item()) == 5.0


@pytest.mark.parametrize("body,kind,shape", [("BODY_LAP3D7_F64", "3d7", (20, 37, 130)), ("BODY_LAP2D5_F64", "2d5", (70, 264))])
def test_builtin_bodies_through_the_c_abi(nh, body, kind, shape):
    body_id = getattr(nh.capi, body)
    u = helpers.hash_field(shape, np.float64, seed=64)
    want = helpers.oracle_entry(kind, u)
    bounds = ([1] * len(shape), [n - 1 for n in shape])
    ref, bound = cc.dot_terms(want, u, mc.inside_slices(shape, [0] * len(shape), bounds))
    F = nh.fields.DeviceField
    fin = F.from_numpy(u)
    cf, K = nh.apply.make_cfg, nh.capi
    for cfg in (None, cf(K.KERNEL_DIRECT), cf(K.KERNEL_MARCH, 0, 3)):
        out = F.empty_like(fin)
        out.tensor.fill_(SENTINEL)
        d = nh.apply.apply_dot(body_id, [fin], out, bounds, cfg=cfg)
        assert d is not None and bits_equal(out.numpy(), want), mismatch_report(out.numpy(), want)
        assert abs(d - ref) <= bound
    # the device scalar of the asynchronous form, and the refusals of neptune_hip_apply_builtin
    dst = nh.torch.zeros(1, dtype=nh.torch.float64, device="cuda")
    out = F.empty_like(fin)
    assert nh.apply.apply_dot(body_id, [fin], out, bounds, dot_out=dst) is dst
    nh.torch.cuda.synchronize()
    assert abs(float(dst.item()) - ref) <= bound
    g = nh.apply.geom_for([fin], out, bounds)
    arr = (C.c_void_p * 1)(fin.ptr)
    st = nh.fields.current_stream_ptr()
    assert nh.lib.neptune_hip_apply_builtin_dot(body_id, C.byref(g), arr, out.ptr, out.ptr + 8, st, None) == K.EINVAL
    assert nh.lib.neptune_hip_apply_builtin_dot(body_id, C.byref(g), arr, fin.ptr, dst.data_ptr(), st, None) == K.EINVAL
    assert nh.lib.neptune_hip_apply_builtin_dot(99, C.byref(g), arr, out.ptr, dst.data_ptr(), st, None) == K.EINVAL
