"""The one bridge stream (csrc/runtime/solver_host.hpp): the step loops, the Krylov solvers and the multigrid drivers all stand
in for the legacy default stream with the same internal stream, so a sequence of them issued on the default stream, with
torch kernels before and after and no host synchronisation in between, must be ordered exactly like the same sequence on
an explicit stream.

Sequence: a torch kernel fills x; apply.step_loop takes STEPS steps (not blocking); multigrid.solve runs two cycles on the
result; apply.cg_solve; multigrid.cg_solve (or cg_solve_mixed) with max_iters=3, check_every=2; a torch kernel reads x.
The solvers block on the bridge stream themselves, so the sequence ends with the two edges once more where nothing else
waits: a torch kernel writes x, a second step loop of STEPS launches (not blocking) starts from it at once, and a torch
kernel reads its result at once.
Every intermediate field, the final field, every returned scalar and the three launch counters must be equal, bit for bit,
between the run on the legacy default stream and the run on a non-default torch stream.

Problem: rank 2, box 17 x 17, Omega 15 x 15, three vertex-centred levels 15, 7, 3 of mg_cases.mg_module (the unscaled
Poisson star), minv = 0.8 / 4 on Omega; the step loop iterates monitor_cases.star_module's contraction on the same box."""
import contextlib

import numpy as np
import pytest

import helpers
import mg_cases as mgc
import mg_device as mgd
import monitor_cases as mc
from helpers import bits_equal, mismatch_report

pytestmark = pytest.mark.gpu

OMEGA, LEVELS, DAMP = (15, 15), 3, 0.8
STEPS = 35          # odd: the state ends in the second field; 1 plain launch, two graphs of 16, 2 plain launches
SHAPES = mgc.level_shapes(OMEGA, LEVELS)


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    ns.texts = {dt: ([mgc.mg_module(shape, dt) for shape, _ in SHAPES], mc.star_module(SHAPES[0][0], dt)) for dt in (np.float64, np.float32)}
    # level 0 with its dot entry (the Krylov solvers' fused launch), the coarser levels and the step loop's module plain
    mgd.prefetch([job for levels, step in ns.texts.values() for job in [(levels[0], True), (step, False)] + [(t, False) for t in levels[1:]]])
    return ns


def _hierarchy(nh, dtype):
    """three levels of the star operator on the device, level 0 with its dot entry; every work field NaN"""
    F = nh.fields.DeviceField
    levels = []
    for l, (text, (shape, where)) in enumerate(zip(nh.texts[dtype][0], SHAPES)):
        minv = F.from_numpy(mgc.minv_field(shape, where, dtype, DAMP, outside=0.0 if l == 0 else np.nan))
        levels.append(nh.mg.Level(mgd.entry(nh, text, l == 0), F.from_numpy(np.zeros(shape, dtype)), mgd.bounds(where), minv=minv))
    return mgd.poison(nh, nh.mg.Hierarchy(levels), dtype)


def _sequence(nh, dtype, last, on_stream):
    """-> (the snapshots of the state after every call, the calls' results, the counters)"""
    torch, F = nh.torch, nh.fields.DeviceField
    shape, where = SHAPES[0]
    bounds = mgd.bounds(where)
    h = _hierarchy(nh, dtype)
    step_entry = mgd.entry(nh, nh.texts[dtype][1])
    seed = F.from_numpy(helpers.hash_field(shape, dtype, seed=5))
    b = F.from_numpy(helpers.hash_field(shape, dtype, seed=6))
    x, y, z = (F.from_numpy(np.zeros(shape, dtype)) for _ in range(3))
    nan = lambda dt=dtype: F.from_numpy(np.full(shape, np.nan, dt))
    krylov_work, mg_work = [nan() for _ in range(3)], [nan() for _ in range(3)]
    if last == "mixed":
        inner = mgd.poison(nh, _hierarchy(nh, np.float32), np.float32, held=True)
    torch.cuda.synchronize()   # the set-up is done; from here to the last snapshot nothing but the calls themselves waits

    snaps, results = [], []
    with (torch.cuda.stream(torch.cuda.Stream()) if on_stream else contextlib.nullcontext()):
        assert (nh.fields.current_stream_ptr() != 0) == on_stream
        torch.mul(seed.tensor, 0.5, out=x.tensor)                                      # 1. a torch kernel fills x
        u = nh.apply.step_loop(step_entry, x, y, bounds, STEPS)                         # 2. not blocking
        assert u is y
        snaps.append(u.tensor.clone())
        results.append(nh.mg.solve(h, u, b, max_cycles=2))                              # 3.
        snaps.append(u.tensor.clone())
        results.append(nh.apply.cg_solve(h.levels[0].entry, u, b, bounds, 4, 0.0, work=krylov_work)[:3])   # 4.
        snaps.append(u.tensor.clone())
        if last == "mixed":                                                             # 5.
            res = nh.mg.cg_solve_mixed(h.levels[0], inner, u, b, max_iters=3, check_every=2, trace=True, work=mg_work)
        else:
            res = nh.mg.cg_solve(h, u, b, max_iters=3, check_every=2, trace=True, work=mg_work)
        results.append(res[:3])
        snaps.append(torch.from_numpy(res[3]))
        snaps.append(u.tensor.clone())
        snaps.append(u.tensor * 2 + x.tensor)                                           # 6. a torch kernel reads x
        torch.add(u.tensor, x.tensor, out=x.tensor)                                     # 7. a torch kernel writes x,
        v = nh.apply.step_loop(step_entry, x, z, bounds, STEPS)                         #    a loop not blocking reads it at once
        snaps.append(v.tensor + x.tensor)                                               #    and a torch kernel its result
    torch.cuda.synchronize()
    counts = (nh.mg.counts(), nh.mg.cg_counts(), nh.apply.cg_counts())
    return [t.cpu().numpy() for t in snaps], results, counts


@pytest.mark.parametrize("dtype,last", [(np.float64, "cg"), (np.float32, "cg"), (np.float64, "mixed")], ids=["f64", "f32", "f64_mixed"])
def test_default_stream_sequence_equals_the_explicit_stream_one(nh, dtype, last):
    want_snaps, want_results, want_counts = _sequence(nh, dtype, last, on_stream=True)
    got_snaps, got_results, got_counts = _sequence(nh, dtype, last, on_stream=False)
    print(f"results = {got_results}, counts = {got_counts}")
    # the sequence did run: two cycles and their checks, three MGCG iterations in two blocks, four CG checks, all finite
    assert got_counts[0] == (2, 0, 2) and got_counts[1][0] + got_counts[1][1] == 3 and got_counts[1][3] == 2 and got_counts[2][2] == 4
    assert all(np.isfinite(a).all() for a in got_snaps)
    assert got_results == want_results and got_counts == want_counts
    assert len(got_snaps) == len(want_snaps) == 7
    for k, (got, want) in enumerate(zip(got_snaps, want_snaps)):
        assert bits_equal(got, want), f"snapshot {k}: " + mismatch_report(got, want)
