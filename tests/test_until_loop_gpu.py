"""neptune_hip_step_loop_until: iterate u <- A(u) until S = sum (A(u) - u)^2 <= tol2, S out of the checked
step's own launch.  Operators: contractive star relaxations (f64, absolute weights summing to 0.75, so S falls steadily) --
5-point on 48x264, 7-point on 12x20x136 -- and, for the fallback, two rank-3 stars the plane-in-LDS kernel runs: radius 2
(13-point) and radius 5 (31-point).  The automatic plan of a radius-2 star is the plane-in-LDS kernel only on fields with
256 tiles and more (pick_march_variant sends smaller ones to the small march tile, which HAS a monitored form), so on this
test's small field that operator is held to the plane kernel by its tile, cfg = (march, tile 7); the radius-5 star is beyond
the march kernel's registers and runs the plane kernel on the automatic plan at any size.

tol2 is chosen from the oracle: the test steps the oracle, takes S at every check point and sets tol2 to the geometric mean
of two consecutive check values, after requiring that those two differ by at least 5 % -- far above the summation bound
2 (n - 1) eps sum |x_i| (~1e-11 relative here), so the stop step cannot hinge on rounding.  (On these operators consecutive
values differ by a factor of 2 to 5.)"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import monitor_cases as mc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

MAX_ORACLE_STEPS = 13
OPERATORS = {
    "relax5_48x264": ((48, 264), 1),
    "relax7_12x20x136": ((12, 20, 136), 1),
    "star13_12x20x136": ((12, 20, 136), 2),     # plane-in-LDS kernel on tile 7: no monitored form, the loop's fallback
    "star31_14x22x136": ((14, 22, 136), 5),     # plane-in-LDS kernel on the automatic plan
}
PLANE_TILE = 7


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
    ns.cache = {}
    return ns


def _operator(nh, name):
    """-> (entry, bounds, states, sums, bounds_of_sums): the compiled operator and the oracle's run -- states[k] after k
    steps, sums[k] = S of step k (k >= 1) with the bound any other summation order of its terms stays within.  Computed
    once per operator and left unchanged."""
    if name not in nh.cache:
        shape, radius = OPERATORS[name]
        text = mc.star_module(shape, radius=radius)
        mod = nh.lowering.compile_module(text, norm_entries=True)
        entry = mod.norm_entry("entry")
        bounds = ([radius] * len(shape), [n - radius for n in shape])
        where = mc.inside_slices(shape, [0] * len(shape), bounds)
        om = helpers.oracle.Module.parse(text)
        states, sums, errs = [helpers.hash_field(shape, np.float64, seed=5)], [None], [None]
        for _ in range(MAX_ORACLE_STEPS):
            nxt = np.zeros_like(states[-1])
            om.call("entry", nxt, states[-1])
            s, b = mc.reference_sum(nxt, states[-1], where)
            states.append(nxt)
            sums.append(s)
            errs.append(b)
        for a in states:
            a.setflags(write=False)
        nh.cache[name] = (entry, bounds, states, sums, errs)
    return nh.cache[name]


def _fields(nh, u0):
    F = nh.fields.DeviceField
    a = F.from_numpy(u0)
    b = F.empty_like(a)
    b.tensor.copy_(a.tensor)     # both fields carry the boundary values, as in any ping-pong loop
    return a, b


def _expected_stop(sums, check_every, max_steps, tol2):
    """what the loop's definition gives on the oracle's sums: (steps_done, last S, number of checks)"""
    done, checks = 0, 0
    while done < max_steps:
        done += min(check_every, max_steps - done)
        checks += 1
        if sums[done] <= tol2:
            break
    return done, sums[done], checks


def _tol_between_checks(sums, check_every, which):
    """tol2 = geometric mean of S at check points number `which` and `which` + 1 (1-based), which must differ by >= 5 %"""
    a, b = sums[which * check_every], sums[(which + 1) * check_every]
    assert b <= 0.95 * a, "precondition: consecutive check values differ by at least 5 %"
    return math.sqrt(a * b)


def _check_run(nh, name, check_every, max_steps, tol2, norm="auto", expect_path=None, cfg=None):
    entry, bounds, states, sums, errs = _operator(nh, name)
    a, b = _fields(nh, states[0])
    done, last = nh.apply.step_loop_until(entry, a, b, bounds, max_steps, tol2, check_every=check_every, norm=norm, cfg=cfg)
    want_done, want_sum, want_checks = _expected_stop(sums, check_every, max_steps, tol2)
    fused, fallback, checks = nh.apply.until_loop_counts()
    print(f"{name} check_every={check_every} max_steps={max_steps} tol2={tol2!r}: steps_done={done} (oracle {want_done}) "
          f"last_sum={last!r} (oracle {want_sum!r}, bound {errs[want_done]:.3e}) fused={fused} fallback={fallback} checks={checks}")
    assert done == want_done
    newest, other = ((a, b)[done % 2]).numpy(), ((a, b)[(done + 1) % 2]).numpy()
    assert bits_equal(newest, states[done]), mismatch_report(newest, states[done])
    assert bits_equal(other, states[done - 1]), mismatch_report(other, states[done - 1])   # the last launch is one step
    assert abs(last - want_sum) <= errs[done]
    assert checks == want_checks and fused + fallback == checks
    if expect_path == "fused":
        assert fused == checks and fallback == 0
    elif expect_path == "fallback":
        assert fallback == checks and fused == 0
    return done


@pytest.mark.parametrize("name", ["relax5_48x264", "relax7_12x20x136"])
@pytest.mark.parametrize("check_every", [1, 3])
def test_stops_where_the_oracle_stops(nh, name, check_every):
    """the march plan: every check is a monitored launch"""
    sums = _operator(nh, name)[3]
    tol2 = _tol_between_checks(sums, check_every, 2)
    done = _check_run(nh, name, check_every, MAX_ORACLE_STEPS, tol2, expect_path="fused")
    assert done == 3 * check_every


@pytest.mark.parametrize("name", ["relax5_48x264", "relax7_12x20x136"])
def test_check_every_beyond_max_steps_is_one_shortened_block(nh, name):
    done = _check_run(nh, name, check_every=50, max_steps=7, tol2=1e300, expect_path="fused")
    assert done == 7 and nh.apply.until_loop_counts()[2] == 1


@pytest.mark.parametrize("name", ["relax5_48x264", "relax7_12x20x136"])
def test_max_steps_reached_without_convergence(nh, name):
    assert _check_run(nh, name, check_every=3, max_steps=8, tol2=0.0, expect_path="fused") == 8   # blocks of 3, 3, 2
    assert nh.apply.until_loop_counts()[2] == 3


def test_max_steps_zero_touches_nothing(nh):
    entry, bounds, states, _, _ = _operator(nh, "relax5_48x264")
    a, b = _fields(nh, states[0])
    b.tensor.fill_(-3.0)
    assert nh.apply.step_loop_until(entry, a, b, bounds, 0, 1.0) == (0, 0.0)
    assert bits_equal(a.numpy(), states[0]) and bool((b.tensor == -3.0).all())
    assert nh.apply.until_loop_counts() == (0, 0, 0)


@pytest.mark.parametrize("name,tile", [("star13_12x20x136", PLANE_TILE), ("star31_14x22x136", None)])
@pytest.mark.parametrize("check_every", [1, 3])
def test_plane_in_lds_plan_runs_the_fallback(nh, check_every, name, tile):
    entry, bounds, states, sums, _ = _operator(nh, name)
    cfg = None if tile is None else nh.apply.make_cfg(nh.capi.KERNEL_MARCH, tile)
    # the plan is the plane-in-LDS kernel, which has no monitored form: refused, nothing launched
    a, b = _fields(nh, states[0])
    b.tensor.fill_(-3.0)
    assert nh.apply.apply_norm(entry, [a], b, bounds, cfg=cfg) is None and bool((b.tensor == -3.0).all())
    tol2 = _tol_between_checks(sums, check_every, 2)
    done = _check_run(nh, name, check_every, MAX_ORACLE_STEPS, tol2, expect_path="fallback", cfg=cfg)
    assert done == 3 * check_every


@pytest.mark.parametrize("name", ["relax5_48x264", "star31_14x22x136"])
def test_without_a_norm_entry_the_loop_is_the_fallback(nh, name):
    sums = _operator(nh, name)[3]
    tol2 = _tol_between_checks(sums, 2, 2)
    assert _check_run(nh, name, 2, MAX_ORACLE_STEPS, tol2, norm=None, expect_path="fallback") == 6


def test_builtin_body_loop(nh):
    """fn = NULL: a built-in body through neptune_hip_apply_builtin_norm (the Laplacian is no contraction: S is only
    compared, the loop runs to max_steps)"""
    shape = (48, 264)
    u = helpers.hash_field(shape, np.float64, seed=3)
    bounds = ([1, 1], [47, 263])
    states = [u]
    for _ in range(5):
        states.append(helpers.oracle_entry("2d5", states[-1]))
    ref, bound = mc.reference_sum(states[5], states[4], mc.inside_slices(shape, [0, 0], bounds))
    a, b = _fields(nh, u)
    done, last = nh.apply.step_loop_until(nh.capi.BODY_LAP2D5_F64, a, b, bounds, 5, 0.0, check_every=2)
    assert done == 5 and abs(last - ref) <= bound and nh.apply.until_loop_counts() == (3, 0, 3)
    assert bits_equal(b.numpy(), states[5]) and bits_equal(a.numpy(), states[4])


def _raw_call(nh, entry, a, b, bounds, max_steps, check_every, stream):
    g = nh.apply.geom_for([a], b, bounds)
    fields2 = (C.c_void_p * 2)(a.ptr, b.ptr)
    ins = (C.c_void_p * 1)(a.ptr)
    done, last = C.c_int64(-1), C.c_double(-1.0)
    rc = nh.lib.neptune_hip_step_loop_until(C.cast(entry.fn, C.c_void_p), C.cast(entry.fn_norm, C.c_void_p), -1, a.dtype,
                                            C.byref(g), fields2, ins, max_steps, check_every, 1.0, stream, None,
                                            C.byref(done), C.byref(last))
    return rc, done.value


def test_refusals_leave_the_fields_untouched(nh):
    entry, bounds, states, _, _ = _operator(nh, "relax5_48x264")
    a, b = _fields(nh, states[0])
    b.tensor.fill_(-3.0)
    st = nh.fields.current_stream_ptr()
    assert _raw_call(nh, entry, a, b, bounds, 5, 0, st) == (nh.capi.EINVAL, 0)        # check_every < 1
    assert _raw_call(nh, entry, a, b, bounds, -1, 1, st) == (nh.capi.EINVAL, 0)       # max_steps < 0
    assert _raw_call(nh, entry, a, a, bounds, 5, 1, st) == (nh.capi.EINVAL, 0)        # equal buffers
    # a call while the stream is being captured: the scalar could not be read back
    torch = nh.torch
    side = torch.cuda.Stream()
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        scratch.add_(1.0)
        captured = _raw_call(nh, entry, a, b, bounds, 5, 1, int(side.cuda_stream))
    assert captured == (nh.capi.EINVAL, 0)
    torch.cuda.synchronize()
    assert bits_equal(a.numpy(), states[0]) and bool((b.tensor == -3.0).all())
