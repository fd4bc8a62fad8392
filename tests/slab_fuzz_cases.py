"""Seeded random modules for SLAB MODE (neptune_hip_set_slab, csrc/runtime/lowered_runtime.hpp), the arbitrary
decompositions they run on, and the rank emulation -- no GPU needed to import.  The slab runtime takes
(start, stop, ghost_lo, ghost_hi) as plain numbers, so ONE process can play every rank of a decomposition in turn: the
rank's dense local buffers are cut out of the global arrays (local_inputs), ghost planes included.

gen_slab_module(seed) -> (text, meta): one global box with a logical origin away from 0 (dim 0 included, both signs over
the seed list), element type f64 / f32, rank 1-4, and the functions

    @entry(out, [out1,] in0..)  one stencil apply of the loaded arguments -- star or box footprint, reach along dim 0 drawn
                                from {0, 1, 2, 3} independently of the other axes, 1-3 inputs, apply.bounds at random within
                                the halo margin -- and a whole-buffer or sub-box store.  Group seeds add a sibling apply over
                                shared inputs with a destination of its own: a group off-slab, member by member on a slab.
    @staged(out, in0..)         pointwise apply -> stencil apply on its result -> pointwise apply or explicit time_advance
                                (method 0, pointwise rhs) -> store: the whole_local / stale_ghosts route.
    @total(in0) -> elem         reduce {kind = "sum"} over a declared box of the pointwise apply @terms: inline (the fused
                                apply + reduce kernel) or through apply_nonlinear (a temp, then the fixed-tree sum).
    @terms(in0)                 the opdef of that apply: what the oracle's terms are read from.

Rank 4 comes as a batch of 3-D operators (no offset along dim 0: seed % 10 == 8) and as a stencil in four dimensions (the
rank-generic kernel: seed % 10 == 9).  The generator emits nothing a slab refuses (a refusal is abort() in the caller): one
apply with a reach along dim 0 per function at most, reading arguments or pointwise results of them only; unconditional
accesses inside the global box; reduce kind sum; scalar results the bare reduce.  tests/test_slab_fuzz_host.py asserts that
over `meta`, and makes the coverage of SEEDS x decompositions binding."""
import numpy as np

from test_fuzz_gpu import gen_chain

# 16 modules, 5 of rank >= 3.  seed % 10 -> rank (and the rank-4 form), (seed // 10) % 2 -> element type.
SEEDS = [0, 11, 21, 30, 2, 12, 23, 33, 44, 54, 65, 6, 17, 27, 8, 19]
# the seeds whose @entry apply also runs through the C plan on the loop-back communicator: rank 2 and 3
GEOM_SEEDS = [s for s in SEEDS if s % 10 in (2, 3, 4, 5, 6, 7)]

_RANK_OF = {0: 1, 1: 1, 2: 2, 3: 2, 4: 2, 5: 2, 6: 3, 7: 3, 8: 4, 9: 4}


def seed_rank_elem(seed):
    """-> (rank, elem, rank-4 form or None): they follow from the seed, so that a short list covers every pair"""
    k = seed % 10
    return _RANK_OF[k], ("f64" if (seed // 10) % 2 == 0 else "f32"), ({8: "batch", 9: "nd"}.get(k))


def loopback(local, lo, hi, r, transport):
    """the local buffer after a loop-back exchange of its r ghost planes per side (a communicator of one rank whose
    neighbours are the rank itself): RCCL matches the two send / receive pairs in order, so the lower ghost planes get the
    rank's own FIRST owned planes and the upper ones its LAST; the peer transport pushes to the neighbour's opposite side"""
    ext = local.copy()
    if transport == "rccl":
        ext[:lo], ext[hi:] = local[lo:lo + r], local[hi - r:hi]
    else:
        ext[:lo], ext[hi:] = local[hi - r:hi], local[lo:lo + r]
    return ext


# ---- footprints: the star and box footprints of tests/test_fuzz_gpu.py gen_apply, with the reach along dim 0 drawn on its own
def _footprint(rng, rank, nin, h, form, star=False):
    """-> (accesses [(input, offsets)], box?).  h: reach along dim 0; the other axes reach 1-2 (star) or 1 (box)"""
    r = int(rng.choice([1, 1, 2]))
    box = rank in (2, 3) and rng.random() < 0.35 and not star
    if box:
        r = 1
    reach = [h] + [r] * (rank - 1)
    if form == "batch":
        reach[0] = 0
    axes = [d for d in range(rank) if reach[d] > 0]
    acc = []
    for k in range(nin):
        acc.append((k, (0,) * rank))
        if k > 0 and rng.random() < 0.4:                # read at the centre only
            continue
        if not axes:
            continue
        for n in range(int(rng.integers(3, 7))):
            if box:
                off = tuple(int(rng.integers(-reach[d], reach[d] + 1)) for d in range(rank))
            else:
                d = axes[int(rng.integers(0, len(axes)))]
                if k == 0 and n < 2 and reach[0] > 0:   # input 0 always reaches h along dim 0, both ways
                    d = 0
                a = reach[d] if (n < 2 or rng.random() < 0.5) else 1
                s = (-1, 1)[n % 2] if n < 2 else int(rng.choice([-1, 1]))
                off = tuple(s * a if x == d else 0 for x in range(rank))
            if any(off) and (k, off) not in acc:
                acc.append((k, off))
    if box and reach[0] > 0:                            # the box's corners along dim 0
        for s in (-1, 1):
            off = (s * reach[0],) + tuple(int(rng.choice([-1, 1])) for _ in range(rank - 1))
            if (0, off) not in acc:
                acc.append((0, off))
    return acc, bool(box)


def _body(rng, acc, rank, elem, origin, shape, index_term):
    """region lines of an apply over accesses `acc`: gen_chain, in some an scf.if on a region index with a conditional access
    (one of the accesses it already has, so the reach stays what `acc` says), and -- index_term -- the dim-0 index itself"""
    L, vals = [], []
    for n, (k, off) in enumerate(acc):
        L.append(f"%a{n} = neptune_ir.access %in{k}[{', '.join(map(str, off))}] : !t -> {elem}")
        vals.append(f"%a{n}")
    res, cnt = gen_chain(rng, L, vals, elem)
    if rng.random() < 0.5:
        d = int(rng.integers(0, rank))
        thr = origin[d] + shape[d] // 2
        cnt += 1
        ck, coff = acc[int(rng.integers(0, len(acc)))]
        L += [f"%thr{cnt} = arith.constant {thr} : index", f"%q{cnt} = arith.cmpi slt, %i{d}, %thr{cnt} : index",
              f"%v{cnt} = scf.if %q{cnt} -> ({elem}) {{",
              f"  %ca{cnt} = neptune_ir.access %in{ck}[{', '.join(map(str, coff))}] : !t -> {elem}",
              f"  %cb{cnt} = arith.addf {res}, %ca{cnt} : {elem}", f"  scf.yield %cb{cnt} : {elem}", "} else {",
              f"  %cc{cnt} = arith.subf {res}, {vals[0]} : {elem}", f"  scf.yield %cc{cnt} : {elem}", "}"]
        res = f"%v{cnt}"
    if index_term:                                      # the GLOBAL plane number: a slab's local plane p is start - ghost_lo + p
        cnt += 1
        L += [f"%w{cnt} = arith.index_cast %i0 : index to i64", f"%wf{cnt} = arith.sitofp %w{cnt} : i64 to {elem}",
              f"%v{cnt} = arith.addf {res}, %wf{cnt} : {elem}"]
        res = f"%v{cnt}"
    L.append(f"neptune_ir.yield {res} : {elem}")
    return L


def _pointwise(rng, nin, rank, elem):
    L, vals = [], []
    for k in range(nin):
        L.append(f"%a{k} = neptune_ir.access %in{k}[{', '.join(['0'] * rank)}] : !t -> {elem}")
        vals.append(f"%a{k}")
    if nin == 1:                                        # something to compute: x * x
        L.append(f"%a1 = arith.mulf %a0, %a0 : {elem}")
        vals.append("%a1")
    res, _ = gen_chain(rng, L, vals, elem)
    L.append(f"neptune_ir.yield {res} : {elem}")
    return L


def _reach(acc, rank):
    lo = [max([0] + [-o[d] for _, o in acc]) for d in range(rank)]
    hi = [max([0] + [o[d] for _, o in acc]) for d in range(rank)]
    return lo, hi


def _bounds_within(rng, origin, shape, lo, hi, extra0):
    """apply.bounds at random within the halo margin; dim 0 up to `extra0` planes tighter, so that cuts fall inside it"""
    rank = len(shape)
    lb = [origin[d] + lo[d] + int(rng.integers(0, 2 if d else extra0 + 1)) for d in range(rank)]
    ub = [origin[d] + shape[d] - hi[d] - int(rng.integers(0, 2 if d else extra0 + 1)) for d in range(rank)]
    return lb, ub


def _sub_box(rng, origin, shape, extra0):
    rank = len(shape)
    lb = [origin[d] + int(rng.integers(0, 3 if d else extra0 + 1)) for d in range(rank)]
    ub = [origin[d] + shape[d] - int(rng.integers(0, 3 if d else extra0 + 1)) for d in range(rank)]
    return lb, ub


def _draw(seed):
    rank, elem, form = seed_rank_elem(seed)
    rng = np.random.default_rng(7919 * seed + 3)
    vk = 2 if elem == "f64" else 4
    h = 0 if form == "batch" else int(rng.choice([0, 1, 2, 3]))
    if form == "nd":
        h = max(h, 1)                                   # the four-dimensional stencil reads neighbouring planes
    group = rank in (2, 3) and seed % 10 in (4, 5, 7)
    rows = [64 * vk - 1, 64 * vk, 64 * vk + 1, 128 * vk, 128 * vk + vk + 1, 37, 50]      # ragged, aligned, shorter than a wave
    if rank == 1:
        shape = [int(rng.integers(2000, 5000))]
    else:
        n0 = int(rng.integers(max(8, 4 * (h + 2)), 41)) if rank < 4 else int(rng.integers(8, 15))
        mid = [int(rng.integers(7, 13)) if rank < 4 else int(rng.integers(5, 8)) for _ in range(rank - 2)]
        last = rows[int(rng.integers(0, len(rows)))] if rank < 4 else [37, 50, 64 * vk + 1][int(rng.integers(0, 3))]
        shape = [n0] + mid + [int(last)]
    origin = [int(rng.integers(-5, 8))] + [int(rng.integers(-3, 5)) for _ in range(rank - 1)]
    if seed % 3 == 0 and origin[0] >= 0:
        origin[0] = -origin[0] - 2
    extra0 = 3 if rank > 1 else 40
    fns = {}
    # ---- @entry
    nin = int(rng.integers(1, 4))
    acc, box = _footprint(rng, rank, nin, h, form, star=group)
    lo, hi = _reach(acc, rank)
    e = dict(nin=nin, acc=acc, box=box, halo0=max(lo[0], hi[0]),
             body=_body(rng, acc, rank, elem, origin, shape, index_term=rng.random() < 0.7),
             bounds=_bounds_within(rng, origin, shape, lo, hi, extra0),
             store=_sub_box(rng, origin, shape, 2 * extra0) if rng.random() < 0.5 else None)
    if group:                                           # the sibling: same bounds, shared input 0, no reach along dim 0
        acc1 = [(0, (0,) * rank)] + [(0, tuple(s if x == rank - 1 else 0 for x in range(rank))) for s in (-1, 1)]
        if nin > 1:
            acc1.append((1, (0,) * rank))
        e["sibling"] = dict(nin=min(nin, 2), acc=acc1, body=_body(rng, acc1, rank, elem, origin, shape, index_term=False))
        lo1, hi1 = _reach(acc1, rank)
        lo, hi = [max(a, b) for a, b in zip(lo, lo1)], [max(a, b) for a, b in zip(hi, hi1)]
        e["bounds"] = _bounds_within(rng, origin, shape, lo, hi, extra0)
    fns["entry"] = e
    # ---- @staged: pointwise -> stencil -> pointwise | time_advance
    nin_s = int(rng.integers(1, 3))
    hs = h if rng.random() < 0.7 else int(rng.integers(0, h + 1))
    if form == "nd":
        hs = max(hs, 1)
    acc_s, box_s = _footprint(rng, rank, nin_s, hs, form)
    lo, hi = _reach(acc_s, rank)
    whole = (list(origin), [o + n for o, n in zip(origin, shape)])
    fns["staged"] = dict(nin=nin_s, acc=acc_s, box=box_s, halo0=max(lo[0], hi[0]),
                         pre=_pointwise(rng, nin_s, rank, elem),
                         pre_bounds=whole if rng.random() < 0.5 else _sub_box(rng, origin, shape, 2),
                         body=_body(rng, acc_s, rank, elem, origin, shape, index_term=rng.random() < 0.5),
                         bounds=_bounds_within(rng, origin, shape, lo, hi, extra0),
                         last="time_advance" if rng.random() < 0.5 and elem == "f64" else "pointwise",   # (explicit: f64 only)
                         post=_pointwise(rng, 2, rank, elem), rhs=_pointwise(rng, 1, rank, elem),
                         post_bounds=whole if rng.random() < 0.5 else _sub_box(rng, origin, shape, 2),
                         store=_sub_box(rng, origin, shape, 2 * extra0) if rng.random() < 0.4 else None)
    # ---- @total: sum over a declared box of a pointwise apply
    n0 = shape[0]
    red = _sub_box(rng, origin, shape, max(n0 // 3, 1))
    fns["total"] = dict(nin=1, halo0=0, body=_pointwise(rng, 1, rank, elem), bounds=_sub_box(rng, origin, shape, extra0),
                        reduce=red, form="fused" if (seed // 10) % 2 == (seed % 2) and rank < 4 else "plain")
    return dict(seed=seed, rank=rank, elem=elem, form=form, group=group, origin=origin, shape=shape, fns=fns)


def _bounds(b):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, b[0]))}], ub = [{', '.join(map(str, b[1]))}]>"


def _apply(res, operands, bounds, rank, body, indent="    "):
    tys = ", ".join(["!t"] * len(operands))
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    ins = ", ".join(f"%in{k}: !t" for k in range(len(operands)))
    return ([f"{indent}{res} = neptune_ir.apply({', '.join(operands)}) attributes {{bounds = {_bounds(bounds)}}} : ({tys}) -> !t {{",
             f"{indent}  ^bb0({idx}, {ins}):"] + [f"{indent}    " + l for l in body] + [f"{indent}}}"])


def _store(val, dst, box):
    if box is None:
        return f"    neptune_ir.store {val} to {dst} : !t to !f"
    return f"    neptune_ir.store {val} to {dst} {{bounds = {_bounds(box)}}} : !t to !f"


def _text(c, plain=False):
    """plain: @entry's store a whole-buffer one, so that what it leaves in `out` is the apply's raw result"""
    rank, elem, fns = c["rank"], c["elem"], c["fns"]
    mr = "x".join("?" * rank) + "x" + elem
    gbox = (c["origin"], [o + n for o, n in zip(c["origin"], c["shape"])])
    T = ['#l = #neptune_ir.location<"cell">', "#b = " + _bounds(gbox),
         f"!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>",
         f"!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>", "module {"]
    t, s = fns["total"], fns["staged"]
    T += ["  neptune_ir.nonlinear_opdef @terms : (!t) -> !t {", "  ^bb0(%u0: !t):"] + _apply("%r", ["%u0"], t["bounds"], rank, t["body"]) + \
         ["    neptune_ir.return %r : !t", "  }"]
    if s["last"] == "time_advance":
        T += ["  neptune_ir.nonlinear_opdef @rhs : (!t) -> !t {", "  ^bb0(%u0: !t):"] + \
             _apply("%r", ["%u0"], s["post_bounds"], rank, s["rhs"]) + ["    neptune_ir.return %r : !t", "  }"]

    def head(name, outs, nin, result):
        args = [f"%{o}: memref<{mr}>" for o in outs] + [f"%m{k}: memref<{mr}>" for k in range(nin)]
        L = [f"  func.func @{name}(" + ", ".join(args) + f") -> {result} {{"]
        for o in outs:
            L.append(f"    %f{o} = neptune_ir.wrap %{o} : memref<{mr}> -> !f")
        for k in range(nin):
            L += [f"    %f{k} = neptune_ir.wrap %m{k} : memref<{mr}> -> !f", f"    %t{k} = neptune_ir.load %f{k} : !f -> !t"]
        return L

    def tail(out):
        return [f"    %res = neptune_ir.unwrap %f{out} : !f -> memref<{mr}>", f"    func.return %res : memref<{mr}>", "  }"]
    e = fns["entry"]
    outs = ["out", "out1"] if c["group"] else ["out"]
    T += head("entry", outs, e["nin"], f"memref<{mr}>")
    T += _apply("%y", [f"%t{k}" for k in range(e["nin"])], e["bounds"], rank, e["body"])
    if c["group"]:
        T += _apply("%y1", [f"%t{k}" for k in range(e["sibling"]["nin"])], e["bounds"], rank, e["sibling"]["body"])
    T.append(_store("%y", "%fout", None if plain else e["store"]))
    if c["group"]:
        T.append(_store("%y1", "%fout1", None))
    T += tail("out")
    T += head("staged", ["out"], s["nin"], f"memref<{mr}>")
    T += _apply("%p", [f"%t{k}" for k in range(s["nin"])], s["pre_bounds"], rank, s["pre"])
    T += _apply("%s", ["%p"] + [f"%t{k}" for k in range(1, s["nin"])], s["bounds"], rank, s["body"])
    if s["last"] == "time_advance":
        T += ["    %dt = arith.constant 0.125 : f64",
              "    %q = neptune_ir.time_advance %s, %dt {method = 0 : i32, rhs = @rhs} : !t, f64 -> !t"]
    else:
        T += _apply("%q", ["%s", "%t0"], s["post_bounds"], rank, s["post"])
    T.append(_store("%q", "%fout", s["store"]))
    T += tail("out")
    T += head("total", [], 1, elem)
    if t["form"] == "fused":
        T += _apply("%sq", ["%t0"], t["bounds"], rank, t["body"])
    else:
        T.append("    %sq = neptune_ir.apply_nonlinear @terms(%t0) : (!t) -> !t")
    T += [f"    %sum = neptune_ir.reduce %sq in {_bounds(t['reduce'])} {{kind = \"sum\"}} : !t -> {elem}", f"    func.return %sum : {elem}", "  }", "}"]
    return "\n".join(T) + "\n"


def _meta(c):
    fns = c["fns"]
    box = lambda b: None if b is None else (list(b[0]), list(b[1]))
    return {
        "seed": c["seed"], "rank": c["rank"], "elem": c["elem"], "form": c["form"], "group": c["group"],
        "origin": list(c["origin"]), "shape": list(c["shape"]),
        "halo0": {k: f["halo0"] for k, f in fns.items()},
        "nin": {k: f["nin"] for k, f in fns.items()},
        "outs": {"entry": 2 if c["group"] else 1, "staged": 1, "total": 0},
        "bounds": {k: box(f["bounds"]) for k, f in fns.items()},
        "box_footprint": {"entry": fns["entry"]["box"], "staged": fns["staged"]["box"]},
        "store": {"entry": box(fns["entry"]["store"]), "staged": box(fns["staged"]["store"])},
        "reduce": box(fns["total"]["reduce"]), "total_form": fns["total"]["form"], "staged_last": fns["staged"]["last"],
        # every apply of a function, in order: (reach along dim 0, reads only arguments / pointwise results of them)
        "applies": {"entry": [fns["entry"]["halo0"]] + ([0] if c["group"] else []),
                    "staged": [0, fns["staged"]["halo0"], 0],
                    "total": [0] if fns["total"]["form"] == "fused" else []},      # (plain: the apply is @terms')
        "other_input_reaches_dim0": any(k > 0 and o[0] != 0 for k, o in fns["entry"]["acc"]),
    }


def gen_slab_module(seed):
    c = _draw(seed)
    return _text(c), _meta(c)


def plain_module(seed):
    """the seed's module with a whole-buffer store in @entry: the oracle's view of what the apply's geometry-level entry
    computes (LoweredModule.geom_entry("entry"))"""
    return _text(_draw(seed), plain=True)


def np_dtype(meta):
    return np.float64 if meta["elem"] == "f64" else np.float32


def inputs(meta, n):
    import helpers
    return [helpers.hash_field(tuple(meta["shape"]), np_dtype(meta), seed=1000 * meta["seed"] + 41 * k + 9) for k in range(n)]


# ---- decompositions: arbitrary cuts, built with Slab(...) directly ----
def _cut(slab_mod, meta, radius, widths):
    g0 = meta["origin"][0]
    glb, gub = tuple(meta["origin"]), tuple(o + n for o, n in zip(meta["origin"], meta["shape"]))
    world, out, start = len(widths), [], g0
    assert sum(widths) == meta["shape"][0] and (world == 1 or min(widths) >= radius)
    for r, w in enumerate(widths):
        out.append(slab_mod.Slab(rank=r, world=world, radius=radius, glb=glb, gub=gub, start=start, stop=start + w,
                                 r_lo=radius if r > 0 else 0, r_hi=radius if r < world - 1 else 0))
        start += w
    return out


def _widths(rng, n0, world, radius, forced):
    """`world` widths >= radius that add up to n0; forced: {rank: width}"""
    w = [forced.get(r, radius) for r in range(world)]
    free = [r for r in range(world) if r not in forced]
    rest = n0 - sum(w)
    assert rest >= 0 and (free or rest == 0)
    for _ in range(rest if rest < 64 else 0):
        w[free[int(rng.integers(0, len(free)))]] += 1
    if rest >= 64:                                      # rank 1: thousands of cells
        parts = sorted(int(x) for x in rng.integers(0, rest + 1, len(free) - 1))
        for r, (a, b) in zip(free, zip([0] + parts, parts + [rest])):
            w[r] += b - a
    return w


def decompositions(meta, seed):
    """a few decompositions per seed, each a list of Slab (one per rank): every rank owns at least `radius` planes (the
    exchange's own contract), `radius` is the greatest reach along dim 0 of the module's functions plus 0, 1 or 2 (at least
    1), and over SEEDS they hold world 1 to 5, a rank exactly `radius` planes thick, one between radius + 1 and 2 radius
    planes thick, and cuts inside the first / last planes of the apply, store and reduce boxes"""
    from neptune_hip import slab as slab_mod
    rng = np.random.default_rng(104729 * seed + 11)
    n0 = meta["shape"][0]
    H = max(meta["halo0"].values())
    out = []
    # (1) radius = the reach itself; world 1..5 by seed; one rank exactly `radius` planes thick, at an edge or inside
    r1 = max(H, 1)
    world = min(1 + seed % 5, n0 // (2 * r1))
    where = [0, world - 1, world // 2][seed % 3]
    out.append(_cut(slab_mod, meta, r1, _widths(rng, n0, world, r1, {where: r1} if world > 1 else {0: n0})))
    # (2) one more ghost plane than the apply reads; a rank between one and two halos thick
    r2 = max(H, 1) + 1
    world = max(2, min(2 + (seed // 2) % 3, n0 // (2 * r2)))
    thin = int(rng.integers(r2 + 1, 2 * r2 + 1))
    out.append(_cut(slab_mod, meta, r2, _widths(rng, n0, world, r2, {int(rng.integers(0, world)): thin})))
    # (3) two more; the first cut strictly inside the planes before the apply's bounds, or the last one behind them, where
    # the box leaves room (that rank then makes zero trips), thin ranks of both kinds beside it
    r3 = max(H, 1) + 2
    if n0 >= 4 * r3:
        world = max(2, min(3 + seed % 2, n0 // (2 * r3)))
        forced = {0: r3, world - 1: int(rng.integers(r3 + 1, 2 * r3 + 1))} if seed % 2 else \
                 {world - 1: r3, 0: int(rng.integers(r3 + 1, 2 * r3 + 1))}
        if world == 2:
            forced.pop(0 if seed % 2 == 0 else 1)
        out.append(_cut(slab_mod, meta, r3, _widths(rng, n0, world, r3, forced)))
    return out


def local_inputs(slab, global_arrays, poison):
    """the rank's dense local buffers: planes [start - r_lo, stop + r_hi) of the global arrays; poison: NaN ghost planes"""
    g0 = slab.glb[0]
    lo, hi = slab.owned_planes()
    out = []
    for g in global_arrays:
        loc = np.ascontiguousarray(g[slab.local_lb[0] - g0:slab.local_ub[0] - g0]).copy()
        if poison:
            loc[:lo] = np.nan
            loc[hi:] = np.nan
        out.append(loc)
    return out


def clipped(slab, box):
    """a declared box cut to the rank's owned planes -> (lb, ub), ub[0] >= lb[0]; a box that is empty along any dimension
    makes zero trips"""
    lb, ub = list(box[0]), list(box[1])
    lb[0], ub[0] = max(lb[0], slab.start), min(ub[0], slab.stop)
    ub[0] = max(ub[0], lb[0])
    return lb, ub


def trips(box):
    n = 1
    for a, b in zip(*box):
        n *= max(b - a, 0)
    return n
