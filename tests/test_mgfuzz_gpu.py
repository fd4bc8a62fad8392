"""multigrid.solve, cg_solve (with and without line stages on level 0) and cg_solve_mixed on the fuzzed hierarchies of
tests/mgfuzz_cases.py against its composed NumPy restatement: one test per seed.

No reduction enters a field, so every field is compared bit for bit on its whole box, the cells outside Omega included:
after solve() x_0 and every level's x_l, b_l; for the CG forms the restatement's recurrences, driven by the device's rz_0 and
traced scalars, must reproduce x, r, p, z (mixed: r32 and z32 as well) and every coarser x_l, b_l.  rr_0, every rr read after
a block and every traced scalar must lie within 2 (n - 1) eps sum |t_i| of the exact sum of the restatement's own terms
(mg_cases.residual, cg_cases.dot_terms, mgcgmixed_cases.wide_dot_terms).  The counts must be those of the launch path, a
quarter of the seeds run the other path as well and must give identical bits, and the inputs (b, minv, the factor fields)
must be unchanged.  Every work field holds NaN before the call.  A refused case must raise and leave every field as it was."""
import copy
import time

import numpy as np
import pytest

import mg_device as mgd
import mgfuzz_cases as fz
import solver_trace_cases as stc
from helpers import bits_equal, mismatch_report
from mg_device import entry as _entry, same as _same

pytestmark = pytest.mark.gpu

SEEDS = fz.SEEDS


@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    ns = mgd.namespace(tmp_path_factory.mktemp("neptune_cache"))
    jobs = dict.fromkeys(job for seed in SEEDS for job in fz.case_modules(fz.decode(seed)))
    t0 = time.perf_counter()
    mgd.prefetch(jobs)
    print(f"\nprefetched {len(jobs)} modules in {time.perf_counter() - t0:.1f} s")
    return ns


class Device:
    """a case on the device: h (the hierarchy), x, b, work, outer (mixed), and `inputs`: [(name, field, host array)] of
    everything the call may only read"""


def _device(nh, B, stages=None, m0_region=None):
    """every work field holds NaN; level 0's streamed fields start case["offset"] bytes into larger allocations.  stages:
    per level the stage axes to build instead of the case's (the refused cases); m0_region: level 0's launch region instead"""
    c = B.case
    F = nh.fields.DeviceField
    outer_dt = fz.D if c["form"] == "mixed" or c.get("why") == "mixed_stage0" else c["dtype"]

    def make0(a):
        off = c["offset"] // a.itemsize
        return stc.offset_field(nh, a.copy(), off) if off else F.from_numpy(a.copy())      # (x0 and b are read-only)
    nan = lambda shape, dt: np.full(shape, np.nan, dt)
    dev = Device()
    dev.inputs = []
    modules = fz.case_modules(c)
    if outer_dt != c["dtype"]:
        (text64, dot), modules = modules[0], modules[1:]
        dev.outer = nh.mg.Level(_entry(nh, text64, dot), F.from_numpy(np.zeros(c["shapes"][0], fz.D)), c["bounds"][0],
                                region=fz.region_of(c, 0))
    levels = []
    for l, R in enumerate(B.levels):
        axes = [s[0] for s in R.stages] if stages is None else stages[l]
        lines = []
        for s, axis in enumerate(axes):
            _, lo, inv, up = R.stages[s] if stages is None else fz.stage_factors(R.shape, R.where, R.weights, min(axis, c["rank"] - 1), c["dtype"])
            fields = [F.from_numpy(a) for a in (lo, inv, up)]
            dev.inputs += [(f"{nm}_{l}[{s}]", f, a) for nm, f, a in zip(("lo", "inv", "up"), fields, (lo, inv, up))]
            lines.append(nh.mg.LineStage(min(axis, c["rank"] - 1), *fields))
        minv = None
        if not lines or c["seed"] % 2:          # a level with stages does not read minv: given or not, by the seed's parity
            minv = make0(R.minv) if l == 0 else F.from_numpy(R.minv)
            dev.inputs.append((f"minv_{l}", minv, R.minv))
        region = m0_region if (l == 0 and m0_region) else fz.region_of(c, l)
        text, dot = modules[l]
        levels.append(nh.mg.Level(_entry(nh, text, dot), F.from_numpy(np.zeros(R.shape, c["dtype"])), c["bounds"][l], minv=minv,
                                  rscale=R.rscale, region=region, lines=lines))
    dev.levels = levels
    dev.x, dev.b = make0(B.x0), make0(B.b)
    dev.inputs.append(("b", dev.b, B.b))
    dev.work = [make0(nan(B.x0.shape, B.x0.dtype)) for _ in range(3)]
    return dev


def _hierarchy(nh, B, dev):
    c = B.case
    # mixed: z32 and r32 are level 0's x and b
    dev.h = h = mgd.poison(nh, nh.mg.Hierarchy(dev.levels), c["dtype"], c["offset"], held=hasattr(dev, "outer"))
    if not c.get("why"):
        want_halved = [tuple(a) if k == "H" else () for a, k in zip(c["transferred"], c["kinds"])]
        assert h.coarsened == [tuple(a) for a in c["transferred"]] and h.halved == want_halved
        assert [tuple(L.m) for L in h.levels] == c["m"] and [tuple(L.lo) for L in h.levels] == c["lo"]
    return h


class Run:
    pass


def _run(nh, B, graph, monkeypatch):
    """one call on fresh device fields along the launch path `graph`; -> everything it left behind, as host arrays"""
    c = B.case
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "1" if graph else "0")       # read at every call
    dev = _device(nh, B)
    h = _hierarchy(nh, B, dev)
    R = Run()
    if c["form"] == "solve":
        R.res = nh.mg.solve(h, dev.x, dev.b, pre=c["pre"], post=c["post"], coarse_sweeps=c["coarse_sweeps"], max_cycles=c["n"],
                            check_every=c["check_every"], tol2=-1.0)     # no r . r stops it, not even one that underflows to 0
        nh.torch.cuda.synchronize()
        R.counts = nh.mg.counts()
    else:
        kw = dict(sweeps=c["sweeps"], coarse_sweeps=c["coarse_sweeps"], max_iters=c["n"], check_every=c["check_every"], trace=True,
                  work=dev.work, tol2=-1.0)
        if c["form"] == "mixed":
            R.res = nh.mg.cg_solve_mixed(dev.outer, h, dev.x, dev.b, **kw)
        else:
            R.res = nh.mg.cg_solve(h, dev.x, dev.b, lines=h.has_lines, **kw)
        nh.torch.cuda.synchronize()
        R.counts, R.rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
        R.work = [f.numpy() for f in dev.work]
    R.x = dev.x.numpy()
    R.xs = [f.numpy() if f is not None else None for f in h.x]
    R.bs = [f.numpy() if f is not None else None for f in h.b]
    for name, field, want in dev.inputs:
        got = field.numpy()
        assert bits_equal(got, want), f"the input {name} changed: " + mismatch_report(got, want)
    return R


def _check_solve(B, R):
    c = B.case
    done, rr0, rr_last, rr_checks = R.res
    ref_rr0, ref_checks = fz.reference(B)
    assert done == c["n"]
    assert R.counts == fz.expected_counts(c), R.counts
    # b_0 is an input (_run holds it unchanged): R.bs[0] is None
    mgd.compare((ref_rr0, ref_checks, [L.x for L in B.levels], [L.b for L in B.levels]), rr0, rr_checks, [R.x] + R.xs[1:], R.bs)
    assert rr_last == rr_checks[-1]


def _check_cg(B, R):
    c = B.case
    V = copy.copy(R)                    # the run as mg_device.compare_replay reads it: named fields, the coarser levels alone
    V.fields = dict(zip("rp", R.work))
    if c["form"] == "mixed":
        V.fields.update(r32=R.bs[0], z32=R.xs[0])
    else:
        V.fields["z"] = R.work[2]
    V.xs, V.bs = R.xs[1:], R.bs[1:]
    mgd.compare_replay(V, B.problem, B.x0, B.b, c["n"], c["check_every"], fz.expected_counts(c), any_fallback=True,
                       sweeps=c["sweeps"], coarse_sweeps=c["coarse_sweeps"])


def _check_refused(nh, B, monkeypatch):
    """the Python layer refuses the combination (ValueError); handed past it, the library refuses it with
    NEPTUNE_HIP_EINVAL (stages on level 0 under mixed precision: NEPTUNE_HIP_EUNSUPPORTED, as the header says) and launches
    nothing: every field keeps its bits"""
    c = B.case
    why, rank = c["why"], c["rank"]
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "1" if c["graph"] else "0")
    kw = dict(coarse_sweeps=c["coarse_sweeps"], check_every=c["check_every"])

    def fields_of(dev):
        out = [("x", dev.x), ("b", dev.b)] + [(f"work[{i}]", f) for i, f in enumerate(dev.work)]
        for nm in ("x", "b", "q"):
            out += [(f"{nm}_{l}", f) for l, f in enumerate(getattr(dev.h, nm)) if f is not None]
        return out + [(nm, f) for nm, f, _ in dev.inputs]

    def unchanged(dev, before):
        nh.torch.cuda.synchronize()
        for (nm, f), want in zip(fields_of(dev), before):
            _same(nm, f.numpy(), want)

    if why == "stage_axis":
        dev = _device(nh, B, stages=[[], [0]])
        st = dev.levels[1].lines[0]
        with pytest.raises(ValueError):
            nh.mg.Level(dev.levels[1].entry, dev.levels[1].like, c["bounds"][1], minv=dev.levels[1].minv, lines=[st._replace(axis=rank)])
        h = _hierarchy(nh, B, dev)
        before = [f.numpy() for _, f in fields_of(dev)]
        dev.levels[1].lines[0] = st._replace(axis=rank)             # past the Python check: the library's own refusal
        with pytest.raises(nh.capi.NeptuneHipError) as err:
            nh.mg.solve(h, dev.x, dev.b, max_cycles=c["n"], **kw)
        assert err.value.code == nh.capi.EINVAL
        with pytest.raises(nh.capi.NeptuneHipError) as err:
            nh.mg.cg_solve(h, dev.x, dev.b, max_iters=c["n"], work=dev.work, lines=True, **kw)
        assert err.value.code == nh.capi.EINVAL
        unchanged(dev, before)
    elif why == "mixed_kinds":
        dev = _device(nh, B)
        with pytest.raises(ValueError, match="mixes two grid kinds"):
            nh.mg.Hierarchy(dev.levels)
        # a hierarchy the Python layer accepts -- dimension 0 cut to the coarse extent by level 0's region: kept -- whose
        # level 0 then gets the case's region back: dimension 0 halved and dimension 1 coarsened in one pair
        lo, m1 = c["lo"][0], c["m"][1]
        wide = fz.region_of(c, 0)
        cut = ([lo[0]] + wide[0][1:], [lo[0] + m1[0]] + wide[1][1:])
        dev = _device(nh, B, m0_region=cut)
        h = _hierarchy(nh, B, dev)
        assert h.halved == [()] and h.coarsened == [(1,)]
        before = [f.numpy() for _, f in fields_of(dev)]
        g = dev.levels[0].geom
        g.region_lb[0], g.region_ub[0] = wide[0][0], wide[1][0]
        with pytest.raises(nh.capi.NeptuneHipError) as err:
            nh.mg.solve(h, dev.x, dev.b, max_cycles=c["n"], **kw)
        assert err.value.code == nh.capi.EINVAL
        with pytest.raises(nh.capi.NeptuneHipError) as err:
            nh.mg.cg_solve(h, dev.x, dev.b, max_iters=c["n"], work=dev.work, **kw)
        assert err.value.code == nh.capi.EINVAL
        unchanged(dev, before)
    else:
        assert why == "mixed_stage0"
        dev = _device(nh, B)
        h = _hierarchy(nh, B, dev)
        assert h.levels[0].lines and h.dtype == nh.capi.F32
        before = [f.numpy() for _, f in fields_of(dev)]
        with pytest.raises(ValueError, match="line stages on level 0"):
            nh.mg.cg_solve_mixed(dev.outer, h, dev.x, dev.b, max_iters=c["n"], work=dev.work, **kw)
        unchanged(dev, before)

        class Unseen(list):             # level 0's stages, which the Python check does not see and the C structs still carry
            def __bool__(self):
                return False
        h.levels[0].lines = Unseen(h.levels[0].lines)
        assert h.has_lines and h._line_structs()[0].n_stages == 1
        with pytest.raises(nh.capi.NeptuneHipError) as err:
            nh.mg.cg_solve_mixed(dev.outer, h, dev.x, dev.b, max_iters=c["n"], work=dev.work, **kw)
        assert err.value.code == nh.capi.EUNSUPPORTED       # the header's answer to stages on level 0; nothing is launched
        unchanged(dev, before)


@pytest.mark.parametrize("seed", SEEDS, ids=[f"s{s:04d}" for s in SEEDS])
def test_seed(nh, seed, monkeypatch):
    t0 = time.perf_counter()
    c = fz.decode(seed)
    print("\n" + fz.describe(seed))
    B = fz.build(c)
    if c["form"] == "refused":
        _check_refused(nh, B, monkeypatch)
        return
    check = _check_solve if c["form"] == "solve" else _check_cg
    R = _run(nh, B, c["graph"], monkeypatch)
    check(B, R)
    if c["both_paths"]:                 # the other launch path on the same inputs: identical bits
        O = _run(nh, B, not c["graph"], monkeypatch)
        assert O.res[:3] == R.res[:3] and (c["form"] == "solve" and O.res[3] == R.res[3] or bits_equal(O.res[3], R.res[3]))
        assert c["form"] == "solve" or O.rz0 == R.rz0
        assert O.counts[0] + O.counts[1] == c["n"] and (O.counts[1] == 0) == (c["graph"] or c["n"] < 3)
        pairs = [("x", O.x, R.x)] + [(f"x_{l}", a, b) for l, (a, b) in enumerate(zip(O.xs, R.xs)) if a is not None]
        pairs += [(f"b_{l}", a, b) for l, (a, b) in enumerate(zip(O.bs, R.bs)) if a is not None]
        pairs += [(f"work[{i}]", a, b) for i, (a, b) in enumerate(zip(getattr(O, "work", []), getattr(R, "work", [])))]
        for nm, a, b in pairs:
            _same(nm + " (the other launch path)", a, b)
    print(f"seed {seed}: {time.perf_counter() - t0:.2f} s")
