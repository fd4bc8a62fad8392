"""The device half of the multigrid GPU tests, once: the session namespace, compiling, problems and their
references, NaN-poisoned hierarchies, the solve / replay runs and their comparison against tests/mg_restatement.py, and the
geometry-only levels and hashed fields of the kernel tests.

A plain module, imported by tests/test_mg*_gpu.py.  Each of those keeps its problems, its parametrisations, its sizes,
seeds, offsets and expected counts, and the assertions that belong to its feature; what they all enforce -- bits equal on
every level's x_l and b_l, every read-back scalar within the restatement's 2 (n - 1) eps sum |t_i|, the launch counts -- is
written here.  Where the files differ in what they assert, the difference is a parameter and each file passes its own.

Nothing here touches the GPU at import; every function takes the namespace `nh` of the calling file's fixture."""
import numpy as np

import helpers
import mg_restatement as rst
import solver_trace_cases as stc
from helpers import bits_equal, mismatch_report


def same(name, got, want):
    assert bits_equal(got, want), f"{name}: " + mismatch_report(got, want)


# ================================================================ the session namespace and compiling
class Namespace:
    pass


def namespace(cache_dir=None, check=()):
    """what every `nh` fixture holds: torch, the package's modules, the loaded and initialised library, the empty entry and
    problem caches.  cache_dir: where this file's modules are compiled to (NEPTUNE_CACHE_DIR).  check: which of a device
    hierarchy's properties hierarchy() holds against the restatement's pairs -- "coarsened", "halved", "linear", "transfers"."""
    import os
    import torch
    assert torch.cuda.is_available()
    if cache_dir is not None:
        os.environ["NEPTUNE_CACHE_DIR"] = str(cache_dir)
    from neptune_hip import _capi, apply, fields, lowering, multigrid
    ns = Namespace()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering, ns.mg = torch, _capi, apply, fields, lowering, multigrid
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    ns.entries, ns.cache, ns.check = {}, {}, tuple(check)
    return ns


def prefetch(jobs):
    """every (text, dot_entries) pair compiled once, side by side, by helpers.prefetch_modules (host threads only, nothing is
    loaded); the dot entries are a lowering option, so another cache key.  12 workers: below the GPU machines' 16 CPUs."""
    from neptune_hip import lowering
    helpers.prefetch_modules([lowering.with_options(text, dot_entries=bool(dot)) for text, dot in dict.fromkeys(jobs)], workers=12)


def entry(nh, text, dot=False):
    """the module's entry, loaded once: with its dot-monitored launch (what MGCG takes on level 0) or the plain geometry-level one"""
    key = (text, bool(dot))
    if key not in nh.entries:
        nh.entries[key] = (nh.lowering.compile_module(text, dot_entries=True).dot_entry("entry") if dot else
                           nh.lowering.compile_module(text).geom_entry("entry"))
    return nh.entries[key]


# ================================================================ problems and references
class Problem:
    """ref: the restatement's levels; texts: a module per level; rests: per level the operator's fixed inputs 1.. (host arrays,
    or device fields kept across runs); entries; x0, b: read-only; dtype; faces; lines: what levels() takes where the caller
    names none; runs: what reference() and the tests cache"""
    faces = lines = None


def finish(nh, P, dots=()):
    """the rest of a problem from its ref, texts, x0 and b: rests (default none), the entries (those not given: level l with
    its dot entry where l is in `dots`), x0 and b read-only, the empty cache"""
    n = len(P.ref)
    if not hasattr(P, "rests"):
        P.rests = [[] for _ in range(n)]
    given = getattr(P, "entries", [None] * n)
    P.entries = [e if e is not None else entry(nh, P.texts[l], l in dots) for l, e in enumerate(given)]
    for a in (P.x0, P.b):
        a.setflags(write=False)
    P.runs = {}
    return P


def problem(nh, key, build, dots=()):
    """the compiled operators, the restatement's levels, x0 and b: built once per key by build(P), x0 and b left unchanged"""
    if key not in nh.cache:
        P = Problem()
        build(P)
        nh.cache[key] = finish(nh, P, dots)
    return nh.cache[key]


def reference(P, cycles, check_every=1, n_levels=None, **kw):
    """the restatement's run, computed once per schedule and left unchanged: -> (rr0, checks, [x_l], [b_l])"""
    key = (cycles, check_every, n_levels, tuple(sorted(kw.items())))
    if key not in P.runs:
        levels = P.ref[:n_levels] if n_levels else P.ref
        rr0, checks = rst.run(levels, P.x0, P.b, cycles, check_every=check_every, **kw)
        P.runs[key] = (rr0, checks, [L.x.copy() for L in levels], [L.b.copy() for L in levels])
    return P.runs[key]


def cached(P, key, make):
    if key not in P.runs:
        P.runs[key] = make()
    return P.runs[key]


# ================================================================ hierarchies
def where_of(lo, m):
    return tuple(slice(l, l + n) for l, n in zip(lo, m))


def bounds(where):
    return [s.start for s in where], [s.stop for s in where]


def outside_of(shape, where):
    mask = np.ones(shape, bool)
    mask[where] = False
    return mask


def dev(nh, a, offset=0):
    """`a` on the device; offset: that many BYTES into a larger allocation"""
    elems = offset // a.itemsize
    return stc.offset_field(nh, a, elems) if offset else nh.fields.DeviceField.from_numpy(a)


def transfer_settings(pair):
    """Level's prolong= / restrict= / faces= for a pair of the restatement with its transfers chosen (none for the others)"""
    if getattr(pair, "rim", None) is None:
        return {}
    out = dict(prolong=pair.prolong, restrict=pair.restrict)
    if pair.prolong == "linear" or pair.restrict == "linear":
        out["faces"] = rst.faces_of(pair.rim)
    return out


def stages_of(nh, R):
    """the restatement level's line stages as device LineStages"""
    F = nh.fields.DeviceField
    return [nh.mg.LineStage(ax, F.from_numpy(lo), F.from_numpy(inv), F.from_numpy(up)) for ax, lo, inv, up in getattr(R, "stages", [])]


def levels(nh, P, n_levels=None, lines=None, constant=False, offset=0):
    """P's levels on the device.  lines: "stages" -- the restatement's own stages, and a level that has some gets no minv --
    or a callback lines(l, entry, like, bounds, others) -> the level's LineStages (minv stays).  constant: every pair with
    the default transfers whatever the restatement's pair says.  offset: level 0's minv that many bytes into a larger
    allocation."""
    F = nh.fields.DeviceField
    lines = lines or P.lines
    out = []
    for l, R in enumerate(P.ref[:n_levels] if n_levels else P.ref):
        like = F.from_numpy(np.zeros(R.shape, P.dtype))
        others = [a if isinstance(a, F) else F.from_numpy(a) for a in P.rests[l]]
        if lines == "stages":
            stages = stages_of(nh, R)
            minv = None if stages else R.minv
        else:
            stages = lines(l, P.entries[l], like, bounds(R.where), others) if lines else ()
            minv = R.minv
        if minv is not None:
            minv = dev(nh, minv, offset if l == 0 else 0)
        setting = {} if constant else transfer_settings(getattr(R, "axes", None))
        out.append(nh.mg.Level(P.entries[l], like, bounds(R.where), others=others, minv=minv, rscale=R.rscale, lines=stages, **setting))
    return out


def poison(nh, h, dtype, offset=0, held=False):
    """NaN into every work field of the hierarchy: q_l, and x_l, b_l for l >= 1; level 0's q `offset` bytes into a larger
    allocation.  held: level 0's x and b as well (mixed precision: they are z32 and r32), else None (the caller's)"""
    nan = lambda f, off=0: dev(nh, np.full(f.shape, np.nan, dtype), off)
    first = [nan(h.q[0], offset), nan(h.q[0], offset)] if held else [None, None]
    h.q = [nan(f, offset if l == 0 else 0) for l, f in enumerate(h.q)]
    h.x = first[:1] + [nan(f) for f in h.x[1:]]
    h.b = first[1:] + [nan(f) for f in h.b[1:]]
    return h


def hierarchy(nh, P, n_levels=None, lines=None, constant=False, offset=0):
    """a device hierarchy whose work fields hold NaN; -> (h, x, b, [r, p, z]).  Held against the restatement's pairs: what
    nh.check names.  offset: level 0's fields and the work fields start that many bytes into larger allocations."""
    h = nh.mg.Hierarchy(levels(nh, P, n_levels, lines, constant, offset))
    pairs = [rst.axes_of(R) for R in (P.ref[:n_levels] if n_levels else P.ref)[:-1]]
    if "coarsened" in nh.check:
        assert h.coarsened == [tuple(p) for p in pairs]
    if "halved" in nh.check:
        assert h.halved == [tuple(p) if p.halved else () for p in pairs]
    if "linear" in nh.check:
        assert [L.linear for L in h.levels[:-1]] == [p.prolong == "linear" and not constant for p in pairs]
    if "transfers" in nh.check:
        assert [(L.linear, L.restrict_linear) for L in h.levels[:-1]] == [(p.prolong == "linear", p.restrict == "linear") for p in pairs]
    poison(nh, h, P.dtype, offset)
    work = [dev(nh, np.full(h.q[0].shape, np.nan, P.dtype), offset) for _ in range(3)]
    return h, dev(nh, P.x0, offset), dev(nh, P.b, offset), work


def mixed(nh, P64, P32):
    """f64 conjugate gradients on P64's level 0 around the f32 cycle of P32's hierarchy, every work field NaN:
    -> (outer, inner, x, b, [r, p, q])"""
    outer = levels(nh, P64)[0]
    inner = poison(nh, nh.mg.Hierarchy(levels(nh, P32)), np.float32, held=True)
    work = [dev(nh, np.full(P64.x0.shape, np.nan)) for _ in range(3)]
    return outer, inner, dev(nh, P64.x0), dev(nh, P64.b), work


def fields_of(h, x, b):
    """-> ([x_l], [b_l]) as host arrays"""
    return [x.numpy()] + [f.numpy() for f in h.x[1:]], [b.numpy()] + [f.numpy() for f in h.b[1:]]


# ================================================================ the solve: running and comparing
def solve(nh, P, max_cycles, tol2=0.0, check_every=1, n_levels=None, lines=None, constant=False, **kw):
    """-> (res, xs, bs, counts)"""
    h, x, b, _ = hierarchy(nh, P, n_levels, lines, constant)
    res = nh.mg.solve(h, x, b, max_cycles=max_cycles, tol2=tol2, check_every=check_every, **kw)
    nh.torch.cuda.synchronize()
    return (res,) + fields_of(h, x, b) + (nh.mg.counts(),)


def compare(ref, rr0, rr_checks, xs, bs):
    """rr_0 and every check within its bound, bits on every x_l and b_l (a field given as None is not the run's to compare)"""
    ref_rr0, ref_checks, ref_x, ref_b = ref
    print(f"rr0 = {rr0!r} (terms' sum {ref_rr0[0]!r}, bound {ref_rr0[1]:.3e})")
    assert abs(rr0 - ref_rr0[0]) <= ref_rr0[1]
    assert len(rr_checks) == len(ref_checks)
    for k, (got, (want, bound)) in enumerate(zip(rr_checks, ref_checks)):
        print(f"  check {k}: rr = {got!r} (terms' sum {want!r}, bound {bound:.3e})")
        assert abs(got - want) <= bound
    for nm, gots, wants in (("x", xs, ref_x), ("b", bs, ref_b)):
        for l, (got, want) in enumerate(zip(gots, wants)):
            if got is not None:
                same(f"{nm}_{l}", got, want)


def check_against_reference(nh, P, cycles, check_every=1, n_levels=None, want_counts=None, **kw):
    """`cycles` cycles with no tolerance against the restatement's run; -> (xs, bs)"""
    (done, rr0, rr_last, rr_checks), xs, bs, counts = solve(nh, P, cycles, check_every=check_every, n_levels=n_levels, **kw)
    sw = {k: v for k, v in kw.items() if k in ("pre", "post", "coarse_sweeps")}
    ref = reference(P, cycles, check_every, n_levels, **sw)
    assert done == cycles and len(rr_checks) == len(ref[1]) == -(-cycles // check_every)
    if want_counts is not None:
        assert counts == want_counts, counts
    compare(ref, rr0, rr_checks, xs, bs)
    assert rr_last == rr_checks[-1]
    return xs, bs


def graph_vs_plain(nh, P, monkeypatch, n, **kw):
    """n cycles by the replayed graph and by plain launches: the counts of each path, identical results and bits, and the
    restatement's x_0"""
    monkeypatch.delenv("NEPTUNE_HIP_MG_GRAPH", raising=False)
    res_g, xs_g, bs_g, counts_g = solve(nh, P, n, **kw)
    monkeypatch.setenv("NEPTUNE_HIP_MG_GRAPH", "0")          # read at every call
    res_p, xs_p, bs_p, counts_p = solve(nh, P, n, **kw)
    assert counts_g == (1, n - 1, n) and counts_p == (n, 0, n)
    assert res_g == res_p
    for a, b in zip(xs_g + bs_g, xs_p + bs_p):
        assert bits_equal(a, b), mismatch_report(a, b)
    assert bits_equal(xs_p[0], reference(P, n)[2][0])


def stop_schedule(P, sequence, check_every, between):
    """a threshold between two values of the restatement's r . r sequence (computed once by sequence()):
    -> (seq, tol2, the most cycles or iterations to allow, (where the definition stops, after how many checks))"""
    seq = cached(P, "seq", sequence)
    tol2 = rst.tol_between(seq, *between)
    limit = len(seq) - 1
    want = rst.expected_stop(seq, check_every, limit, tol2)
    assert want[0] == between[1]
    return seq, tol2, limit, want


def check_stop(nh, P, check_every, between, cycles=6, label="", **kw):
    """solve() with a tolerance stops where the definition says; -> (tol2, the cycles done)"""
    seq, tol2, max_cycles, (want_done, want_checks) = stop_schedule(P, lambda: rst.rr_sequence(P.ref, P.x0, P.b, cycles), check_every, between)
    (done, rr0, rr_last, rr_checks), _, _, counts = solve(nh, P, max_cycles, tol2=tol2, check_every=check_every, **kw)
    print(f"{label}seq = {seq}, tol2 = {tol2!r}, done = {done}, checks = {rr_checks}")
    assert (done, counts[2], len(rr_checks)) == (want_done, want_checks, want_checks)
    assert counts[0] + counts[1] == done
    assert rr_last == rr_checks[-1] <= tol2 and all(v > tol2 for v in rr_checks[:-1])
    return tol2, done


# ================================================================ MGCG: running and comparing
class Run:
    """what an MGCG call left behind, as host arrays: res, x, b, fields (name -> array: r, p, z, or r, p, q, r32, z32 in mixed
    precision; also attributes), xs / bs (the coarser x_l / b_l), q, counts, rz0; h: the device hierarchy"""


def record(nh, res, h, x, b, named):
    R = Run()
    R.res, R.h, R.x, R.b = res, h, x.numpy(), b.numpy()
    R.fields = {nm: f.numpy() for nm, f in named}
    for nm, a in R.fields.items():
        setattr(R, nm, a)
    R.xs = [f.numpy() for f in h.x[1:]]
    R.bs = [f.numpy() for f in h.b[1:]]
    R.q = [f.numpy() for f in h.q]
    R.counts, R.rz0 = nh.mg.cg_counts(), nh.mg.cg_rz0()
    return R


def cg(nh, P, max_iters, tol2=0.0, check_every=1, trace=True, offset=0, b=None, stages=None, require=None, **kw):
    """cg_solve on a fresh poisoned hierarchy; b: another right-hand side; stages: hierarchy()'s lines=; require(h): what
    the hierarchy must be before the call; -> the Run"""
    h, x, bf, work = hierarchy(nh, P, lines=stages, offset=offset)
    assert require is None or require(h)
    if b is not None:
        bf.tensor.copy_(nh.torch.from_numpy(np.ascontiguousarray(b)))
    res = nh.mg.cg_solve(h, x, bf, max_iters=max_iters, tol2=tol2, check_every=check_every, trace=trace, work=work, **kw)
    nh.torch.cuda.synchronize()
    return record(nh, res, h, x, bf, zip("rpz", work))


def check_sums(rr0, rz0, trace, rr0_ref, rz0_ref, checks):
    """rr_0, rz_0 and every traced scalar within the bound of the replay's own terms"""
    print(f"rr0 = {rr0!r} (terms' sum {rr0_ref[0]!r}, bound {rr0_ref[1]:.3e})  rz0 = {rz0!r} (sum {rz0_ref[0]!r}, bound {rz0_ref[1]:.3e})")
    assert abs(rr0 - rr0_ref[0]) <= rr0_ref[1] and abs(rz0 - rz0_ref[0]) <= rz0_ref[1]
    for k, sums in enumerate(checks):
        print(f"  k={k}: " + "  ".join(f"{nm} = {trace[k][c]!r} (sum {s!r}, bound {bd:.3e})"
                                        for c, (nm, (s, bd)) in enumerate(zip(("pq", "rz'", "rr'"), sums))))
        for c, (s, bd) in enumerate(sums):
            assert abs(float(trace[k][c]) - s) <= bd, (k, c, trace[k][c], s, bd)


def check_levels(xs, bs, ref_levels):
    """bits on the coarser x_l, b_l (xs[0] is level 1's) against what the replay left in the restatement's levels"""
    for l, (got_x, got_b, L) in enumerate(zip(xs, bs, ref_levels[1:]), 1):
        same(f"x_{l}", got_x, L.x)
        same(f"b_{l}", got_b, L.b)


def compare_replay(R, problem, x0, b, iters, check_every=1, want_counts=None, any_fallback=False, outside=False, **sweeps):
    """a traced run of `iters` iterations against the restatement's recurrences driven by the run's own scalars (problem: a
    list of levels, or a mixed problem): the trace's shape, the counts, rr_0, rz_0 and every traced scalar within its bound,
    rr_last, and bits on x, the work fields and every coarser x_l, b_l.  any_fallback: want_counts is (plain, graph, checks).
    outside: also x unchanged outside Omega, b unchanged, the other fields +0 outside Omega.  -> the replay's State"""
    done, rr0, rr_last, trace = R.res
    assert done == iters and trace.shape == (iters, 3)
    assert R.counts[0] + R.counts[1] == iters and R.counts[3] == -(-iters // check_every)
    if any_fallback:
        # counts[2], how many iterations took a plain launch and a separate dot product, is the operator's matter: the
        # dot-monitored launch may refuse a many-input apply, and the replay from the traced scalars holds either way
        print(f"counts = {R.counts}")
        assert (R.counts[0], R.counts[1], R.counts[3]) == want_counts, R.counts
    elif want_counts is not None:
        assert R.counts == want_counts, R.counts
    st, checks, rr0_ref, rz0_ref, _ = rst.replay(problem, x0, b, R.rz0, trace, **sweeps)
    check_sums(rr0, R.rz0, trace, rr0_ref, rz0_ref, checks)
    assert rr_last == float(trace[-1][2])
    R.checks = checks
    mixed_form = rst.is_mixed(problem)
    names = ("r", "p", "r32", "z32") if mixed_form else ("r", "p", "z")
    same("x", R.x, st.x)
    for nm in names:
        same(nm, R.fields[nm], getattr(st, nm))
    check_levels(R.xs, R.bs, problem.levels if mixed_form else problem)
    if outside:
        # cells of x outside Omega are never changed; the other fields are +0 there; b is the caller's
        shape, where = (problem.shape, problem.where) if mixed_form else (problem[0].shape, problem[0].where)
        out = outside_of(shape, where)
        assert bits_equal(R.x[out], x0[out]) and bits_equal(R.b, b)
        for nm in names:
            a = R.fields[nm]
            assert bits_equal(a[out], np.zeros(int(out.sum()), a.dtype))
    return st


def check_replay(nh, P, iters, check_every=1, want_counts=None, any_fallback=False, outside=False, offset=0, stages=None, require=None,
                 **kw):
    """one traced run of `iters` iterations against the restatement's replay; -> the run"""
    R = cg(nh, P, iters, check_every=check_every, offset=offset, stages=stages, require=require, **kw)
    sw = {k: v for k, v in kw.items() if k in ("sweeps", "coarse_sweeps")}
    R.state = compare_replay(R, P.ref, P.x0, P.b, iters, check_every, want_counts, any_fallback, outside, **sw)
    return R


def same_runs(G, Pl):
    """two runs along different launch paths: identical scalars, trace and bits"""
    assert G.res[:3] == Pl.res[:3] and bits_equal(G.res[3], Pl.res[3]) and G.rz0 == Pl.rz0
    assert list(G.fields) == list(Pl.fields)
    for a, b in zip([G.x] + list(G.fields.values()) + G.xs + G.bs, [Pl.x] + list(Pl.fields.values()) + Pl.xs + Pl.bs):
        assert bits_equal(a, b), mismatch_report(a, b)


def check_cg_stop(R, seq, tol2, want, label=""):
    """an untraced MGCG run with a tolerance stopped where the definition says"""
    done, rr0, rr_last = R.res
    print(f"{label}seq = {seq}, tol2 = {tol2!r}, done = {done}, rr_last = {rr_last!r}")
    assert (done, R.counts[3]) == want
    assert R.counts[0] + R.counts[1] == done
    assert rr_last <= tol2 < rr0


def cg_sequence(P, iters, sweeps=2):
    """r . r of the restatement's recurrences (numpy's own sums) down to 1e-16 rr_0, computed once: -> (seq, tol2)"""
    def make():
        rr0 = rst.numpy_mgcg(P.ref, P.x0, P.b, 0, sweeps)[0]
        return rst.numpy_mgcg(P.ref, P.x0, P.b, iters, sweeps, stop_at=1e-16 * rr0), 1e-16 * rr0
    return cached(P, ("cg_seq", sweeps), make)


def check_iteration_count(nh, P, limit, sweeps=2, label=""):
    """to 1e-16 rr_0: the count of the restatement's recurrences, whose r . r at the stop and one iteration before must be a
    factor of 2 either side of the threshold, so that the count cannot hinge on a summation order; -> (n, tol2, rr0, x)"""
    seq, tol2 = cg_sequence(P, limit, sweeps)
    n = len(seq) - 1
    print(f"seq = {seq}, tol2 = {tol2!r}")
    assert 1 <= n < limit and seq[n] <= 0.5 * tol2 and seq[n - 1] >= 2.0 * tol2, "precondition on the restatement"
    h, x, b, work = hierarchy(nh, P)
    kw = {} if sweeps == 2 else dict(sweeps=sweeps)
    done, rr0, rr_last = nh.mg.cg_solve(h, x, b, max_iters=limit, tol2=tol2, work=work, **kw)
    nh.torch.cuda.synchronize()
    print(f"{label}done = {done}, rr0 = {rr0!r}, rr_last = {rr_last!r}")
    assert done == n and rr_last <= tol2 < rr0
    return n, tol2, rr0, x.numpy()


# ================================================================ the kernel tests
def level(nh, shape, dtype, where, **settings):
    """a level that carries geometry only (entry None: the kernels alone never call the operator)"""
    return nh.mg.Level(None, nh.fields.DeviceField.from_numpy(np.zeros(shape, dtype)), bounds(where), **settings)


def unequal_rims(lo, m):
    """a box around Omega (m cells at lo) whose high rim differs from the low one and from dimension to dimension"""
    return tuple(l + n + 1 + d for d, (l, n) in enumerate(zip(lo, m)))


class Geometry:
    """two geometry-only levels from their (box, Omega's lower corner, Omega) triples; axes: the dimensions the pair
    transfers, kept for the test; level_settings (rscale, prolong, restrict, faces) go to the fine level, which owns the pair"""

    def __init__(self, nh, fine, coarse, dtype, axes=None, **level_settings):
        (self.fine_shape, flo, fm), (self.coarse_shape, clo, cm) = fine, coarse
        self.fw, self.cw = where_of(flo, fm), where_of(clo, cm)
        self.dtype, self.axes = dtype, axes
        self.fine = level(nh, self.fine_shape, dtype, self.fw, **level_settings)
        self.coarse = level(nh, self.coarse_shape, dtype, self.cw)


def field(shape, dtype, seed, where=None, outside=None, inside=None):
    """hashed values with -0 sprinkled in; `outside` (e.g. NaN) on every cell that is not in `where`, `inside` on those in it"""
    a = helpers.hash_field(shape, dtype, seed=seed)
    flat = a.reshape(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    if outside is not None:
        keep = a[where].copy()
        a[...] = outside
        a[where] = keep
    if inside is not None:
        a[where] = inside
    return a


def factors(shape, where, axis, dtype, seed):
    """the restatement's factors of a random diagonally dominant T along `axis`: NaN outside Omega, on lo at i = 0 and on up
    at i = m - 1"""
    import mglines_cases as lc
    rng = np.random.default_rng(seed)
    m = tuple(s.stop - s.start for s in where)
    lower, diag, upper = (np.zeros(shape, dtype) for _ in range(3))
    lower[where] = rng.uniform(-1.0, 1.0, m)
    upper[where] = rng.uniform(-1.0, 1.0, m)
    diag[where] = rng.uniform(2.5, 4.0, m) * rng.choice([-1.0, 1.0], m)
    lo, inv, up = lc.factors(lower, diag, upper, where, axis, 0.8, outside=np.nan)
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    lo[tuple(first)] = np.nan
    up[tuple(last)] = np.nan
    return lo, inv, up


def line_problem(box, lo_corner, om, axis, dtype):
    """a line stage's inputs: -> (where, q, b, x, (lo, inv, up)); q and b NaN outside Omega, x with one NaN there"""
    where = where_of(lo_corner, om)
    q = field(box, dtype, 41, where, np.nan)
    b = field(box, dtype, 42, where, np.nan)
    x = field(box, dtype, 43)
    x[tuple(0 for _ in box)] = np.nan                                # a cell outside Omega: it keeps its bits
    return where, q, b, x, factors(box, where, axis, dtype, 7 + axis)
