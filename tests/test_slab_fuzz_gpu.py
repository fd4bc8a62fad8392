"""Slab mode of the lowered runtime (neptune_hip_set_slab: csrc/runtime/lowered_runtime.hpp clip_planes / owned_bounds /
local_box, whole_local, stale_ghosts, run_store, run_reduce, the exchange-beside-interior split of run_apply) against the
oracle, in ONE process on one GPU and without torch.distributed: the runtime takes (start, stop, ghost_lo, ghost_hi) as
plain numbers, so this file plays every rank of every decomposition of tests/slab_fuzz_cases.py in turn, its ghost planes
filled from the global arrays.  The reference is the oracle run once per function on the GLOBAL arrays; nothing in it knows
about slabs.  Every owned plane of every rank must equal the oracle's planes [start, stop) bit for bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import helpers
import slab_fuzz_cases as sfc
from helpers import bits_equal, mismatch_report, oracle

pytestmark = pytest.mark.gpu

SEEDS = sfc.SEEDS
SENTINEL = -7.25            # fills every destination (the oracle's too), so unwritten planes are recognisable
GUARD = 91.5                # fills the planes before and after a destination's local buffer
ENV_KEYS = ("NEPTUNE_HIP_KERNEL", "NEPTUNE_HIP_VARIANT", "NEPTUNE_HIP_CHUNK")


class Case:
    """one seed: module, decompositions, global inputs, and the oracle's results on them -- computed once, never changed"""

    def __init__(self, seed, lowering, torch):
        self.seed = seed
        self.text, self.meta = sfc.gen_slab_module(seed)
        self.decs = sfc.decompositions(self.meta, seed)
        self.mod = lowering.compile_module(self.text)
        meta, dt = self.meta, sfc.np_dtype(self.meta)
        self.dt = dt
        self.tdt = torch.float64 if dt == np.float64 else torch.float32
        self.ins = sfc.inputs(meta, 3)
        self.dev_ins = [torch.from_numpy(a).cuda() for a in self.ins]       # the "neighbours' planes" of the pending view
        m = oracle.Module.parse(self.text)
        self.want = {}
        for fn in ("entry", "staged"):
            for alias in (False, True):
                h_ins = [a.copy() for a in self.ins[:meta["nin"][fn]]]
                outs = [np.full(meta["shape"], SENTINEL, dtype=dt) for _ in range(meta["outs"][fn])]
                if alias:
                    outs[0] = h_ins[0]
                m.call(fn, *outs, *h_ins)
                self.want[fn, alias] = outs
        self.terms = m.call("terms", self.ins[0].copy())
        self.kernels = {fn: [a["kernel"] for a in self.mod.report["applies"] if a["function"] == fn] for fn in ("entry", "staged")}
        if "rhs" in self.mod.signatures:
            self.kernels["staged"] += [a["kernel"] for a in self.mod.report["applies"] if a["function"] == "rhs"]

    def march_settings(self):
        """forced march tiles with chunk seams, for functions all of whose applies can march (a forced march kernel that
        cannot take a launch is an error, and rank-4 sub-fields start wherever the leading index puts them)"""
        tiles = {1: ("0",), 2: ("0", "2"), 3: ("0", "7")}.get(self.meta["rank"], ())
        return [{"NEPTUNE_HIP_KERNEL": "march", "NEPTUNE_HIP_VARIANT": v, "NEPTUNE_HIP_CHUNK": c} for v in tiles for c in ("1", "3")]


@pytest.fixture(scope="module")
def env(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache_slab_fuzz"))
    from neptune_hip import _capi, lowering, slab
    helpers.prefetch_modules([sfc.gen_slab_module(seed)[0] for seed in SEEDS])   # every seed's module, compiled side by side

    class NS:
        pass
    ns = NS()
    ns.torch, ns.lowering, ns.slab, ns.capi = torch, lowering, slab, _capi
    ns.lib = _capi.load()
    ns.lib.neptune_hip_init(0)
    ns.cases = {}
    ns.side = torch.cuda.Stream()
    ns.event = ns.lib.neptune_hip_event_create()
    ns.busy = torch.ones(1 << 24, dtype=torch.float32, device="cuda")
    yield ns
    ns.lib.neptune_hip_event_destroy(ns.event)


def case_of(env, seed):
    if seed not in env.cases:
        env.cases[seed] = Case(seed, env.lowering, env.torch)
    return env.cases[seed]


def _guarded(env, case, shape):
    """a sentinel-filled local destination inside a larger allocation, guard planes on both sides (a whole number of
    16-byte units, so the destination is aligned like a buffer of its own)"""
    torch = env.torch
    g = 64 if len(shape) == 1 else 4
    big = torch.full((shape[0] + 2 * g,) + tuple(shape[1:]), GUARD, dtype=case.tdt, device="cuda")
    out = big[g:g + shape[0]]
    out.fill_(SENTINEL)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return big, out, g


def run_rank(env, case, fn, sl, alias, pending, what):
    """@fn on rank `sl` of a decomposition; checks everything but the stitched result, returns the owned planes per output.
    pending: the ghost planes arrive on a side stream and the runtime is handed their event"""
    torch, lib, meta = env.torch, env.lib, case.meta
    nin, nout = meta["nin"][fn], meta["outs"][fn]
    g0 = meta["origin"][0]
    lo, hi = sl.owned_planes()
    good = sfc.local_inputs(sl, case.ins[:nin], poison=False)
    first = sfc.local_inputs(sl, case.ins[:nin], poison=pending)
    d_ins = [torch.from_numpy(a).cuda() for a in first]
    outs, bigs = [], []
    for j in range(nout):
        if alias and j == 0:
            outs.append(d_ins[0])
            bigs.append(None)
        else:
            big, out, g = _guarded(env, case, sl.local_shape)
            outs.append(out)
            bigs.append((big, g))
    if not pending:
        ret = env.slab.ShardedModule(case.mod, sl).call(fn, *outs, *d_ins, exchange=())       # no process group needed
    else:
        torch.cuda.synchronize()
        with torch.cuda.stream(env.side):
            for _ in range(8):                          # unrelated device work first: the ghosts arrive late
                env.busy.mul_(1.0000001)
            a, b = sl.local_lb[0] - g0, sl.local_ub[0] - g0
            for t, g in zip(d_ins, case.dev_ins):
                if lo:
                    t[:lo].copy_(g[a:a + lo])
                if sl.r_hi:
                    t[hi:].copy_(g[b - sl.r_hi:b])
        lib.neptune_hip_event_record(env.event, C.c_void_p(env.side.cuda_stream))
        assert lib.neptune_hip_set_slab(sl.start, sl.stop, sl.r_lo, sl.r_hi) == 0
        lib.neptune_hip_set_slab_pending(env.event)
        try:
            ret = case.mod.call(fn, *outs, *d_ins)
        finally:
            lib.neptune_hip_clear_slab()
        assert lib.neptune_hip_get_slab_pending() is None, what
    torch.cuda.synchronize()
    assert ret is outs[0], what
    owned = []
    for j in range(nout):
        got = outs[j].cpu().numpy()
        want = case.want[fn, alias][j][sl.start - g0:sl.stop - g0]
        assert bits_equal(got[lo:hi], want), f"{what} out{j}\n" + mismatch_report(got[lo:hi], want)
        owned.append(got[lo:hi])
        if bigs[j] is not None:
            big, g = bigs[j]
            guard = torch.full_like(big[:g], GUARD)
            assert torch.equal(big[:g], guard) and torch.equal(big[-g:], guard), f"{what} out{j}: guard planes written"
            if j == 0 and meta["store"][fn] is not None:    # a sub-box store is clipped to the owned planes
                ghosts = np.concatenate([got[:lo], got[hi:]])
                assert bits_equal(ghosts, np.full(ghosts.shape, SENTINEL, dtype=case.dt)), f"{what}: ghost planes of out stored"
            elif fn == "entry" and meta["applies"][fn][j] > 0:
                # a stencil's bounds are clipped to the owned planes, and outside them a result is its input 0
                ghosts, src = np.concatenate([got[:lo], got[hi:]]), np.concatenate([good[0][:lo], good[0][hi:]])
                assert bits_equal(ghosts, src), f"{what} out{j}: ghost planes are not the copy-through of input 0"
            elif fn == "entry":
                # an apply that stays within its plane is computed on the ghost planes too (whole_local)
                held = case.want[fn, alias][j][sl.local_lb[0] - g0:sl.local_ub[0] - g0]
                assert bits_equal(got, held), f"{what} out{j}: ghost planes\n" + mismatch_report(got, held)
    for k in range(nin):                                # every input, ghosts included, keeps its bits (pending: has them now)
        if alias and k == 0:
            continue
        back = d_ins[k].cpu().numpy()
        assert bits_equal(back, good[k]), f"{what} in{k}\n" + mismatch_report(back, good[k])
    return owned


def run_decomposition(env, case, fn, dec, alias, pending, what):
    meta = case.meta
    g0 = meta["origin"][0]
    stitched = [np.full(meta["shape"], np.nan, dtype=case.dt) for _ in range(meta["outs"][fn])]
    for sl in dec:
        if pending and not (sl.r_lo or sl.r_hi):
            continue
        owned = run_rank(env, case, fn, sl, alias, pending, f"{what} rank {sl.rank}/{sl.world} [{sl.start},{sl.stop}) r={sl.radius}")
        for s, o in zip(stitched, owned):
            s[sl.start - g0:sl.stop - g0] = o
    if not pending or len(dec) > 1:
        for j, s in enumerate(stitched):
            assert bits_equal(s, case.want[fn, alias][j]), f"{what}: stitched out{j}\n" + mismatch_report(s, case.want[fn, alias][j])


class launch_env:
    """NEPTUNE_HIP_KERNEL / _VARIANT / _CHUNK set for a block and put back exactly as they were"""

    def __init__(self, settings):
        self.settings = settings

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ENV_KEYS}
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(self.settings)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("seed", SEEDS)
def test_every_rank_of_every_decomposition_matches_the_oracle(env, seed):
    """(a) the plain slab view, ghosts correct from the start: owned planes bit for bit, unwritten planes keep the sentinel,
    guard planes and inputs untouched, the ranks' planes stitched together are the oracle's whole result; again with the
    destination aliasing input 0"""
    case = case_of(env, seed)
    with launch_env({}):
        for fn in ("entry", "staged"):
            for n, dec in enumerate(case.decs):
                for alias in (False, True):
                    run_decomposition(env, case, fn, dec, alias, False, f"seed {seed} @{fn} dec {n} alias={alias}")


@pytest.mark.parametrize("seed", SEEDS)
def test_launch_forms_on_a_slab(env, seed):
    """(b) the same under NEPTUNE_HIP_KERNEL = direct, direct-flat, and -- where every apply of the function can march -- on
    two march tiles with chunk seams of 1 and 3 planes: a launch region that is a dim-0 sub-range of the local buffer"""
    case = case_of(env, seed)
    for fn in ("entry", "staged"):
        settings = [{"NEPTUNE_HIP_KERNEL": "direct"}, {"NEPTUNE_HIP_KERNEL": "direct-flat"}]
        if all(k == "march" for k in case.kernels[fn]):
            settings += case.march_settings()
        for s in settings:
            with launch_env(s):
                for n, dec in enumerate(case.decs):
                    # (a forced march kernel needs a few lane vectors per row; the rows of a rank-1 slab are its cells)
                    if "NEPTUNE_HIP_VARIANT" in s and case.meta["rank"] == 1 and min(sl.local_shape[0] for sl in dec) < 64:
                        continue
                    run_decomposition(env, case, fn, dec, False, False, f"seed {seed} @{fn} dec {n} {s}")
                    if n == len(case.decs) - 1:
                        run_decomposition(env, case, fn, dec, False, True, f"seed {seed} @{fn} dec {n} pending {s}")


@pytest.mark.parametrize("seed", SEEDS)
def test_exchange_beside_the_interior(env, seed):
    """(c) the pending view (neptune_hip_set_slab_pending, as ShardedModule.call does it): the inputs start with NaN ghost
    planes; a side stream does unrelated work, then copies the neighbours' planes in, and its event is handed to the runtime.
    What this can and cannot show: that the runtime WAITS is only very likely to be seen -- a missing wait reads NaN unless
    the copies happen to have landed.  Deterministic is the geometry: interior and edge launches together produce every
    owned plane exactly right, with ghost planes wider than the apply reads (radius > halo0), on slabs thinner than two
    halos (no interior: wait first), on one-sided ranks and with the destination aliasing input 0; and the event is
    consumed (neptune_hip_get_slab_pending() is None afterwards)."""
    case = case_of(env, seed)
    with launch_env({}):
        for fn in ("entry", "staged"):
            for n, dec in enumerate(case.decs):
                for alias in (False, True):
                    run_decomposition(env, case, fn, dec, alias, True, f"seed {seed} @{fn} dec {n} pending alias={alias}")


@pytest.mark.parametrize("seed", SEEDS)
def test_partial_sums_of_the_ranks(env, seed):
    """(d) @total through the C ABI (set the slab, call, clear -- ShardedModule would all-reduce): each rank's partial against
    math.fsum of the oracle's own terms on the rank's clipped box, within what two summation orders of the same n terms may
    differ by, 2 (n - 1) eps sum |x_i| (tests/test_reduce_gpu.py, monitor_cases.reference_sum), eps of the element type;
    an empty clipped box gives exactly +0; the partials add up to the global sum within the same bound.  Ghost planes are
    NaN: a reduce that reached into them would say so."""
    case = case_of(env, seed)
    meta, lib, torch = case.meta, env.lib, env.torch
    eps = float(np.finfo(case.dt).eps)
    origin = meta["origin"]

    def terms_in(box):
        sub = case.terms[tuple(slice(a - o, max(b, a) - o) for a, b, o in zip(box[0], box[1], origin))]
        flat = [float(v) for v in sub.reshape(-1)]
        return flat, 2.0 * max(len(flat) - 1, 0) * eps * math.fsum(abs(v) for v in flat)
    all_terms, all_bound = terms_in(meta["reduce"])
    with launch_env({}):
        for n, dec in enumerate(case.decs):
            parts = []
            for sl in dec:
                loc = torch.from_numpy(sfc.local_inputs(sl, case.ins[:1], poison=True)[0]).cuda()
                assert lib.neptune_hip_set_slab(sl.start, sl.stop, sl.r_lo, sl.r_hi) == 0
                try:
                    part = case.mod.call("total", loc)
                finally:
                    lib.neptune_hip_clear_slab()
                flat, bound = terms_in(sfc.clipped(sl, meta["reduce"]))
                what = f"seed {seed} dec {n} rank {sl.rank}/{sl.world} [{sl.start},{sl.stop}): {part!r} vs {math.fsum(flat)!r} (bound {bound!r}, {len(flat)} terms)"
                if not flat:
                    assert part == 0.0 and math.copysign(1.0, part) == 1.0, what
                assert abs(part - math.fsum(flat)) <= bound, what
                parts.append(part)
            assert abs(math.fsum(parts) - math.fsum(all_terms)) <= all_bound, f"seed {seed} dec {n}: {parts}"


# ---- geometry-level entries through the C plan (neptune_hip_slab_apply) on the loop-back communicator ----
@pytest.fixture(scope="module", params=["rccl", "peer"])
def comm(request, env):
    c = env.slab.SlabComm(0, 1, transport=request.param)            # a world of one rank: its neighbours are itself
    assert env.lib.neptune_hip_slab_comm_transport(c.ptr).decode() == request.param
    yield c
    c.status()                              # no device-side wait of the peer transport ever timed out
    c.close()


def _geom_slabs(env, meta, radius):
    """two-sided middle slabs -- thick, exactly `radius` planes, between one and two halos -- and the two one-sided edge
    slabs, each a world of one rank inside the seed's global box"""
    g0, n0 = meta["origin"][0], meta["shape"][0]
    glb, gub = tuple(meta["origin"]), tuple(o + n for o, n in zip(meta["origin"], meta["shape"]))
    mk = lambda start, own, lo, hi: env.slab.Slab(rank=0, world=1, radius=radius, glb=glb, gub=gub, start=start, stop=start + own,
                                                  r_lo=lo, r_hi=hi)
    thick = min(2 * radius + 3, n0 - 2 * radius - 1)
    out = [mk(g0 + radius + 1, thick, radius, radius), mk(g0 + radius, radius, radius, radius),
           mk(g0 + radius + 2, min(2 * radius, radius + 1 + meta["seed"] % 2), radius, radius),
           mk(g0, radius + 3, 0, radius), mk(g0 + n0 - radius - 2, radius + 2, radius, 0)]
    assert all(s.local_lb[0] >= g0 and s.local_ub[0] <= g0 + n0 for s in out)
    return out


def _looped(local, sl, r, transport):
    """the local buffer after the loop-back exchange; a one-sided loop-back returns the rank's own edge planes of that side
    on both transports (tests/test_slab_rccl_gpu.py)"""
    lo, hi = sl.owned_planes()
    if sl.r_lo and sl.r_hi:
        return sfc.loopback(local, lo, hi, r, transport)
    ext = local.copy()
    if sl.r_hi:
        ext[hi:] = local[hi - r:hi]
    if sl.r_lo:
        ext[:lo] = local[lo:lo + r]
    return ext


@pytest.mark.parametrize("seed", sfc.GEOM_SEEDS)
def test_geometry_level_entries_through_the_c_plan(env, comm, seed):
    """ShardedApply(slab, mod.geom_entry("entry"), bounds, comm=loop-back) = ONE neptune_hip_slab_apply: exchange on the
    plan's communication stream, interior, edge planes.  radius = the apply's reach along dim 0 or one more; several
    inputs (all exchanged); f32; overlap on and off.  The reference is the oracle on the global arrays the loop-back
    implies; owned planes bit for bit, and the inputs' ghost planes hold exactly the looped-back planes.  Called twice: the
    second call reuses plan, stream and events."""
    from neptune_hip import fields
    case = case_of(env, seed)
    meta, torch = case.meta, env.torch
    plain = oracle.Module.parse(sfc.plain_module(seed))
    entry = case.mod.geom_entry("entry")
    nin = meta["nin"]["entry"]
    assert entry.halo0 == meta["halo0"]["entry"] and entry.num_inputs == nin
    radius = max(entry.halo0, 1) + (seed // 10) % 2
    g0 = meta["origin"][0]
    others = [helpers.hash_field(tuple(meta["shape"]), case.dt, seed=7000 + seed + k) for k in range(nin)]
    for sl in _geom_slabs(env, meta, radius):
        lo, hi = sl.owned_planes()
        locals_ = sfc.local_inputs(sl, case.ins[:nin], poison=True)
        exts = [_looped(a, sl, radius, comm.transport) for a in locals_]
        want_glob = []
        for k, ext in enumerate(exts):
            glob = others[k].copy()
            glob[sl.local_lb[0] - g0:sl.local_ub[0] - g0] = ext
            want_glob.append(glob)
        outs = [np.full(meta["shape"], SENTINEL, dtype=case.dt) for _ in range(meta["outs"]["entry"])]
        plain.call("entry", *outs, *want_glob)
        want = outs[0][sl.start - g0:sl.stop - g0]
        for overlap in (True, False):
            what = f"seed {seed} {comm.transport} [{sl.start},{sl.stop}) ghosts {sl.r_lo}/{sl.r_hi} r={radius} overlap={overlap}"
            fins = [fields.DeviceField.from_numpy(a, sl.local_lb) for a in locals_]
            fout = fields.DeviceField.from_numpy(np.full(sl.local_shape, SENTINEL, dtype=case.dt), sl.local_lb)
            op = env.slab.ShardedApply(sl, entry, tuple(meta["bounds"]["entry"]), comm=comm, peers=(0, 0), overlap=overlap)
            for _ in range(2):
                op(fins, fout)
            torch.cuda.synchronize()
            got = fout.numpy()
            assert bits_equal(got[lo:hi], want), what + "\n" + mismatch_report(got[lo:hi], want)
            ghosts = np.concatenate([got[:lo], got[hi:]])
            assert bits_equal(ghosts, np.full(ghosts.shape, SENTINEL, dtype=case.dt)), what + ": ghost planes of the result written"
            for k, f in enumerate(fins):
                back = f.numpy()
                assert bits_equal(back, exts[k]), f"{what} in{k}\n" + mismatch_report(back, exts[k])
            del op
