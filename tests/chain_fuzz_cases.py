"""Seeded random cases for the kernels that do two or three applies per pass over HBM (csrc/kernels/apply_march2.hpp: the
chain kernel, its rank-2 form and the leapfrog form), as module texts and launch geometries -- no GPU needed.

gen_chain_case(seed) -> (text, meta).  One seed is one MODULE (one compile) and `meta["geometries"]` is a list of launch
geometries for it: the chain entries (<tag>__geom2 / __geom3 / __geomL2) take the field boxes, apply.bounds, the launch
region and the chunk from the caller, so extents around the window seams, short dim-0 extents whose warm-up planes are
clamped, shifted origins, tight and one-cell-thick bounds, plane regions and chunk seams are all reached without another
compile.  The class of a seed is seed // 1000 (CLASSES): the form.  The low digits of a seed fix rank, element type and the
per-axis radii (decode), everything else is drawn from the seed's generator.  tests/test_chain_fuzz_host.py makes what SEEDS
covers binding.

The body is a random IEEE-exact expression (test_fuzz_gpu.gen_chain, dyadic constants) over a star of input 0 (offsets from
test_multihalo_gpu.star, thinned out in some seeds and one-sided in some) and the centre of every further input, damped by
2^-4, plus a weighted sum of every access (test_multihalo_gpu.COEF x 2^-5), times the coefficient fields; some seeds add an
index argument of every dimension and an scf.if on an index.  The forms:
    chain     @entry(out, in0, c...) = one apply; entries fn, fn2, fn3
    euler     the same apply as the rhs of a fused explicit step @step = u + dt * A(u) (neptune_ir.time_advance, which is
              f64 and one input only); entries fn, fn2, fn3 of the step
    leapfrog  @entry(next, cur, prev, c...) = one apply of a two-level scheme; entries fn and fnL2

The window constants below restate March2Geom and the window tables of launch_march2 / launch_march2_rank2 /
launch_apply_leapfrog2 from the header; eligible() restates march2_eligible / march2_rank2_eligible."""
import numpy as np

CLASSES = {0: "chain", 1: "euler", 2: "leapfrog", 3: "refused"}
PATTERNS = {3: [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)], 2: [(1, 1), (2, 1), (1, 2), (2, 2)]}
SENTINEL = -7.0
DT = 0.125                         # the Euler step's time step
THRESHOLD = 4                      # the scf.if's index threshold (logical coordinate)
CELL_BUDGET = 1_500_000

# 20 modules, 10 of rank 3 (the slow compiles), and 3 refused seeds that borrow a module.
SEEDS = [8, 14, 16, 42, 84, 1, 7, 11, 61, 1000, 1068, 1001, 1013, 2000, 2002, 2038, 2003, 2007, 2013, 2025,
         3000, 3001, 3002]
# the module a refused seed borrows (3001 needs a one-sided footprint, 3002 a rank-3 module)
REFUSED_BASE = {3000: 7, 3001: 84, 3002: 2000}
# step loops: two seeds per form
LOOP_SEEDS = [61, 42, 1001, 1068, 2000, 2003]


def seed_class(seed):
    return CLASSES[seed // 1000]


def decode(seed):
    """(form, rank, element type, radii per axis): fixed by the seed's digits, so that a short list covers the matrix"""
    form, n = seed_class(seed), seed % 1000
    rank = 3 if n % 2 == 0 else 2
    elem = "f64" if (n // 2) % 2 == 0 or form == "euler" else "f32"
    pats = PATTERNS[rank]
    return form, rank, elem, pats[(n // 4) % len(pats)]


# ---- the kernels' window arithmetic, restated from csrc/kernels/apply_march2.hpp ----------------------------------------
def geom_consts(elem, radii, ns):
    """March2Geom<T, FP, NS>: radii = (R0, R1, R2) in rank 3, (R0, R2) in rank 2 (FP::R1 == 0 there)"""
    size = 8 if elem == "f64" else 4
    r0, r2 = radii[0], radii[-1]
    r1 = radii[1] if len(radii) == 3 else 0
    vk, g = 16 // size, 64 // size
    hg = max(g // 2, vk)
    mk = (ns * r2 + hg - 1) // hg * hg
    span = 64 * vk
    return dict(VK=vk, G=g, HG=hg, MK=mk, SPAN=span, KEEPK=span - 2 * mk, MJ=ns * r1, WARM=2 * r0 * (ns - 1), R0=r0, R1=r1, R2=r2)


def window(form, rank, radii, nin, ns, march2_env=0):
    """(rows per lane, waves per workgroup) of the kernel the entry launches; None: the entry refuses (rank 3, radius 2, three
    applies); rank 2 has no J window.  march2_env: NEPTUNE_HIP_MARCH2 (only the radius-2 table has a second shape in every
    build)"""
    if rank == 2:
        return (1, 1)
    wide = max(radii) > 1
    if form == "leapfrog":
        assert ns == 2
        return (3, 8) if wide else ((3, 12) if nin == 2 else (4, 8))
    if wide:
        return None if ns != 2 else ((4, 8) if march2_env == 1 else (3, 8))
    return (3, 16) if ns == 2 else (3, 12)


def keepj(form, rank, radii, nin, ns, march2_env=0):
    w = window(form, rank, radii, nin, ns, march2_env)
    if rank == 2 or w is None:
        return None
    return w[0] * w[1] - 2 * ns * radii[1]


def eligible(meta, g):
    """march2_eligible / march2_rank2_eligible on geometry g of the module `meta` (equal boxes and 64-byte aligned buffers are
    how the tests allocate), plus the launchers' own refusal of empty bounds"""
    rank, radii = meta["rank"], meta["radii"]
    G = geom_consts(meta["elem"], radii, 2)["G"]
    size = 8 if meta["elem"] == "f64" else 4
    n, o = g["shape"], g["origin"]
    reg = g["region"] or ([0] * rank, list(n))
    for d in range(1, rank):
        if reg[0][d] != 0 or reg[1][d] != n[d]:
            return False
    if n[-1] % G != 0 or n[-1] < 2 * G or n[0] < 1:
        return False
    if rank == 3 and (n[1] < 8 or n[1] * n[2] * size >= 0x7fffffff):
        return False
    for d in range(rank):
        if g["lb"][d] < g["ub"][d] and (g["lb"][d] - radii[d] < o[d] or g["ub"][d] + radii[d] > o[d] + n[d]):
            return False
    return all(l < u for l, u in zip(g["lb"], g["ub"]))


def leapfrog_capable(rank, radii, nin):
    """leapfrog2_footprint / the emitter's leapfrog_capable for a star of input 0 and centre-only further inputs"""
    if rank == 3:
        return nin <= (2 if max(radii) > 1 else 3)
    return rank == 2


# ---- draws -----------------------------------------------------------------------------------------------------------
def _offsets(rng, rank, radii):
    """-> (offsets of input 0, the centre first; one-sided axis or None).  A thinned star keeps, per axis, one offset at the
    axis' radius; a one-sided axis of radius 2 reaches -2 .. +1 or -1 .. +2"""
    from test_multihalo_gpu import star
    full = star(rank, 2)
    one_sided = None
    twos = [d for d in range(rank) if radii[d] == 2]
    if twos and rng.random() < 0.5:
        one_sided = (twos[int(rng.integers(0, len(twos)))], int(rng.choice([-1, 1])))
    thin = rng.random() < 0.4
    out = [full[0]]
    for off in full[1:]:
        d = next(a for a in range(rank) if off[a])
        if abs(off[d]) > radii[d]:
            continue
        if one_sided and one_sided[0] == d and off[d] == -2 * one_sided[1]:
            continue                                    # the far offset on the short side
        at_radius = abs(off[d]) == radii[d] and (not one_sided or one_sided[0] != d or off[d] == 2 * one_sided[1])
        first_at_radius = at_radius and not any(o[d] and abs(o[d]) == radii[d] for o in out[1:])
        if thin and not first_at_radius and rng.random() < 0.4:
            continue
        out.append(off)
    return out, one_sided


def _draw_module(seed):
    from test_fuzz_gpu import gen_chain
    from test_multihalo_gpu import COEF
    form, rank, elem, radii = decode(seed)
    rng = np.random.default_rng(7919 * seed + 11)
    offs, one_sided = _offsets(rng, rank, radii)
    ncen = int(rng.integers(0, 3))                      # centre-only inputs (the leapfrog's previous state not counted)
    if form == "euler":
        ncen = 0                                        # time_advance: the rhs maps the state alone
    if form == "leapfrog" and rank == 3:
        ncen = min(ncen, 0 if max(radii) > 1 else 1)    # leapfrog2_footprint
    nin = 1 + ncen + (1 if form == "leapfrog" else 0)
    uses_index = bool(rng.random() < 0.5)
    uses_if = bool(rng.random() < 0.4)
    acc = [(0, o) for o in offs] + [(k, (0,) * rank) for k in range(1, nin)]
    L, vals = [], []
    for n, (k, off) in enumerate(acc):
        L.append(f"%a{n} = neptune_ir.access %in{k}[{', '.join(map(str, off))}] : !t -> {elem}")
        vals.append(f"%a{n}")
    res, cnt = gen_chain(rng, L, vals, elem)
    cnt += 1
    L += [f"%damp = arith.constant 0.0625 : {elem}", f"%v{cnt} = arith.mulf %damp, {res} : {elem}"]
    res = f"%v{cnt}"
    # gen_chain's selects, min / max and floor can leave a result that hardly depends on some access (all the more on data of
    # the order 0.01): a weighted sum of every access of the states, distinct dyadic weights, evaluated left to right, keeps
    # each one visible in the result's bits
    for n in range(len(offs) + (1 if form == "leapfrog" else 0)):
        cnt += 1
        L += [f"%lw{cnt} = arith.constant {COEF[n] * 0.03125!r} : {elem}", f"%lm{cnt} = arith.mulf %lw{cnt}, {vals[n]} : {elem}",
              f"%v{cnt} = arith.addf {res}, %lm{cnt} : {elem}"]
        res = f"%v{cnt}"
    # coefficient fields are multiplied in
    for k in range(nin - ncen, nin):
        cnt += 1
        L.append(f"%v{cnt} = arith.mulf {res}, {vals[len(offs) + k - 1]} : {elem}")
        res = f"%v{cnt}"
    if uses_index:                                      # every dimension's index: 2^-(10+d) * i_d
        for d in range(rank):
            cnt += 1
            L += [f"%w{cnt} = arith.index_cast %i{d} : index to i64", f"%wf{cnt} = arith.sitofp %w{cnt} : i64 to {elem}",
                  f"%e{cnt} = arith.constant {2.0 ** -(10 + d)!r} : {elem}", f"%we{cnt} = arith.mulf %e{cnt}, %wf{cnt} : {elem}",
                  f"%v{cnt} = arith.addf {res}, %we{cnt} : {elem}"]
            res = f"%v{cnt}"
    if_dim = None
    if uses_if:                                         # scf.if on an index; its access repeats an unconditional one
        if_dim = int(rng.integers(0, rank))
        cnt += 1
        ck, coff = acc[int(rng.integers(0, len(offs)))]
        L += [f"%thr{cnt} = arith.constant {THRESHOLD} : index",
              f"%q{cnt} = arith.cmpi slt, %i{if_dim}, %thr{cnt} : index",
              f"%v{cnt} = scf.if %q{cnt} -> ({elem}) {{",
              f"  %ca{cnt} = neptune_ir.access %in{ck}[{', '.join(map(str, coff))}] : !t -> {elem}",
              f"  %cb{cnt} = arith.subf {res}, %ca{cnt} : {elem}",
              f"  scf.yield %cb{cnt} : {elem}",
              "} else {",
              f"  %h{cnt} = arith.constant 0.5 : {elem}",
              f"  %cc{cnt} = arith.mulf {res}, %h{cnt} : {elem}",
              f"  scf.yield %cc{cnt} : {elem}",
              "}"]
        res = f"%v{cnt}"
    L.append(f"neptune_ir.yield {res} : {elem}")
    return dict(seed=seed, form=form, rank=rank, elem=elem, radii=tuple(radii), offsets=offs, one_sided=one_sided, ncen=ncen,
                nin=nin, uses_index=uses_index, uses_if=uses_if, if_dim=if_dim, body=L, rng=rng)


def _bounds_attr(lb, ub):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, lb))}], ub = [{', '.join(map(str, ub))}]>"


def module_text(c, shape, origin, lb, ub):
    """the module of draw `c` for fields [origin, origin + shape) and apply.bounds [lb, ub).  The geometry-level entries of
    the compiled module take all of these from the caller; the oracle reads them from the text"""
    rank, elem, nin = c["rank"], c["elem"], c["nin"]
    mr = "x".join("?" * rank) + "x" + elem
    tys = ", ".join(["!t"] * nin)
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    T = ['#l = #neptune_ir.location<"cell">',
         "#b = " + _bounds_attr(origin, [o + n for o, n in zip(origin, shape)]),
         "#bi = " + _bounds_attr(lb, ub),
         f"!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>",
         f"!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>",
         "module {",
         f"  neptune_ir.nonlinear_opdef @op : ({tys}) -> !t {{",
         "  ^bb0(" + ", ".join(f"%u{k}: !t" for k in range(nin)) + "):",
         "    %r = neptune_ir.apply(" + ", ".join(f"%u{k}" for k in range(nin)) + f") attributes {{bounds = #bi}} : ({tys}) -> !t {{",
         f"      ^bb0({idx}, " + ", ".join(f"%in{k}: !t" for k in range(nin)) + "):"]
    T += ["        " + l for l in c["body"]]
    T += ["    }", "    neptune_ir.return %r : !t", "  }",
          f"  func.func @entry(%out: memref<{mr}>, " + ", ".join(f"%m{k}: memref<{mr}>" for k in range(nin)) + f") -> memref<{mr}> {{",
          f"    %fo = neptune_ir.wrap %out : memref<{mr}> -> !f"]
    for k in range(nin):
        T += [f"    %f{k} = neptune_ir.wrap %m{k} : memref<{mr}> -> !f", f"    %t{k} = neptune_ir.load %f{k} : !f -> !t"]
    T += ["    %y = neptune_ir.apply_nonlinear @op(" + ", ".join(f"%t{k}" for k in range(nin)) + f") : ({tys}) -> !t",
          "    neptune_ir.store %y to %fo : !t to !f",
          f"    %res = neptune_ir.unwrap %fo : !f -> memref<{mr}>",
          f"    func.return %res : memref<{mr}>", "  }"]
    if c["form"] == "euler":
        T += [f"  func.func @step(%out: memref<{mr}>, %m0: memref<{mr}>) -> memref<{mr}> {{",
              f"    %fo = neptune_ir.wrap %out : memref<{mr}> -> !f",
              f"    %f0 = neptune_ir.wrap %m0 : memref<{mr}> -> !f",
              "    %t0 = neptune_ir.load %f0 : !f -> !t",
              f"    %dt = arith.constant {DT!r} : f64",
              "    %u1 = neptune_ir.time_advance %t0, %dt {method = 0 : i32, rhs = @op} : !t, f64 -> !t",
              "    neptune_ir.store %u1 to %fo : !t to !f",
              f"    %res = neptune_ir.unwrap %fo : !f -> memref<{mr}>",
              f"    func.return %res : memref<{mr}>", "  }"]
    return "\n".join(T + ["}"]) + "\n"


def _ns_list(c):
    return [2] if c["form"] == "leapfrog" else [2, 3]


def _seam_ns(rng, c):
    """the entry whose windows an extent is drawn around: 3 applies has no rank-3 window at radius 2"""
    ns = _ns_list(c)
    if c["rank"] == 3 and max(c["radii"]) > 1:
        ns = [2]
    return int(ns[int(rng.integers(0, len(ns)))])


def _draw_geometry(rng, c, kind):
    """kind: 'seams' (window seams, zero origin, interior bounds, whole field), 'least' (the shortest legal row, 8 rows, a
    dim-0 extent so short that warm-up planes are clamped, shifted origin), 'tight' (seams again, bounds tighter than the
    interior, shifted origin, a region [a, b) inside the field and a chunk that does not divide it), 'thin' (bounds one cell
    thick along one dimension; a region of one plane, or one that starts above the bounds)"""
    rank, radii, elem, form, nin = c["rank"], c["radii"], c["elem"], c["form"], c["nin"]
    ns = _seam_ns(rng, c)
    gc = geom_consts(elem, radii, ns)
    G, KEEPK, WARM, R0 = gc["G"], gc["KEEPK"], gc["WARM"], gc["R0"]
    KJ = keepj(form, rank, radii, nin, ns)
    kseam = jseam = None
    # ---- extents
    if kind == "least":
        last = 2 * G
    else:
        k, e = int(rng.integers(1, 4)) if kind != "thin" else 1, int(rng.integers(-1, 2))
        last, kseam = k * KEEPK + e * G, (k, e, ns)
    n1 = None
    if rank == 3:
        if kind == "least":
            n1 = 8
        else:
            k, e = int(rng.integers(1, 3)) if kind != "thin" else 1, int(rng.integers(-1, 2))
            n1, jseam = k * KJ + e, (k, e, ns)
            assert n1 >= 8
    small_n0 = kind == "least" or (kind == "thin" and rng.random() < 0.5)
    if small_n0:
        ns_small = max(_ns_list(c)) if not (rank == 3 and max(radii) > 1) else 2
        warm = geom_consts(elem, radii, ns_small)["WARM"]
        n0 = int(rng.integers(2 * R0 + 1, warm + 3))
    elif rank == 3:
        n0 = int(rng.integers(2 * R0 + 4, 15))
    else:
        n0 = int(rng.integers(2 * R0 + 12, 71))
    if kind in ("tight", "thin"):
        n0 = max(n0, 2 * R0 + 4) if not small_n0 else n0
    shape = [n0] + ([n1] if rank == 3 else []) + [last]
    assert int(np.prod(shape)) <= CELL_BUDGET
    origin = [0] * rank if kind == "seams" else [int(rng.integers(-6, 10)) for _ in range(rank)]
    # ---- bounds (logical)
    lo, hi = list(radii), [n - r for n, r in zip(shape, radii)]
    bkind, thin_dim = "interior", None
    if kind == "tight":
        bkind = "tight"
        for d in range(rank):
            room = hi[d] - lo[d] - 1
            a = int(rng.integers(0, min(3, room) + 1))
            b = int(rng.integers(0, min(3, room - a) + 1))
            lo[d], hi[d] = lo[d] + a, hi[d] - b
        if all(l == r and h == n - r for l, h, r, n in zip(lo, hi, radii, shape)):
            lo[rank - 1] += 1
    elif kind == "thin":
        bkind, thin_dim = "thin", int(rng.integers(0, rank))
        at = int(rng.integers(lo[thin_dim], hi[thin_dim]))
        lo[thin_dim], hi[thin_dim] = at, at + 1
    lb, ub = [o + l for o, l in zip(origin, lo)], [o + h for o, h in zip(origin, hi)]
    # ---- launch region along dim 0 (result-physical) and the chunk
    rkind, region = "none", None
    if kind == "tight" and n0 >= 4:
        a = int(rng.integers(1, n0 - 2))
        b = int(rng.integers(a + 2, n0)) if a + 2 < n0 else a + 1
        rkind = "inside" if b - a > 1 else "one_plane"
        region = (a, b)
    elif kind == "thin":
        if rng.random() < 0.5 and hi[0] < n0:
            a = int(rng.integers(hi[0], n0))
            rkind, region = "above_bounds", (a, n0)
        else:
            a = int(rng.integers(1, n0 - 1))
            rkind, region = "one_plane", (a, a + 1)
    elif kind == "least" and rng.random() < 0.5:
        a = int(rng.integers(1, n0 - 1))
        rkind, region = "one_plane", (a, a + 1)
    chunks = [1, 2, 3, 5] if rank == 3 else [4, 7, 33]
    chunk = int(chunks[int(rng.integers(0, len(chunks)))])
    if region and rkind == "inside":                    # prefer a chunk that leaves a ragged last chunk inside the region
        ragged = [ch for ch in chunks if ch < region[1] - region[0] and (region[1] - region[0]) % ch]
        if ragged:
            chunk = int(ragged[int(rng.integers(0, len(ragged)))])
    full_region = None if region is None else ([region[0]] + [0] * (rank - 1), [region[1]] + shape[1:])
    return dict(kind=kind, shape=shape, origin=origin, lb=lb, ub=ub, bounds_kind=bkind, thin_dim=thin_dim, region_kind=rkind,
                region=full_region, chunk=chunk, k_seam=kseam, j_seam=jseam, refused=None)


def _never_read(c, g):
    """per input: the cells no stage of any chain reads arithmetically.  A chain's stage reads input 0 (or the stage before,
    which equals input 0 outside the bounds) at bounds + offsets, and the centre-only inputs (a leapfrog's previous state
    included) inside the bounds; every other cell is only ever copied through"""
    shape, rank = g["shape"], c["rank"]
    lo = [l - o for l, o in zip(g["lb"], g["origin"])]
    hi = [u - o for u, o in zip(g["ub"], g["origin"])]
    read0 = np.zeros(shape, dtype=bool)
    for off in c["offsets"]:
        read0[tuple(slice(l + o, h + o) for l, h, o in zip(lo, hi, off))] = True
    inside = np.zeros(shape, dtype=bool)
    inside[tuple(slice(l, h) for l, h in zip(lo, hi))] = True
    return [~read0] + [~inside for _ in range(c["nin"] - 1)]


def _refused_case(seed):
    """geometries no chain entry takes, on a module borrowed from another seed: the entries return EUNSUPPORTED"""
    base = REFUSED_BASE[seed]
    c = _draw_module(base)
    rng = np.random.default_rng(7919 * seed + 11)
    g = _draw_geometry(rng, c, "seams")
    gc = geom_consts(c["elem"], c["radii"], 2)
    rank = c["rank"]
    why = {3000: "ragged_row", 3001: "reach_leaves_box", 3002: "region_dim1"}[seed]
    if why == "ragged_row":                              # a row that is not a whole 64-byte granule
        g["shape"][-1] = 3 * gc["G"] + gc["VK"]
        g["ub"][-1] = g["origin"][-1] + g["shape"][-1] - c["radii"][-1]
    elif why == "reach_leaves_box":                      # in range for the accesses the body makes, not for the symmetric radius
        d, side = c["one_sided"]
        if side > 0:                                     # reaches -1 .. +2: the bounds may start one cell in
            g["lb"][d] = g["origin"][d] + 1
        else:
            g["ub"][d] = g["origin"][d] + g["shape"][d] - 1
    else:                                                # a launch region restricted along dim 1
        g["region"] = ([0] * rank, [g["shape"][0], g["shape"][1] - 2] + g["shape"][2:])
        g["region_kind"] = "dim1"
    g["refused"] = why
    g["kind"] = "refused"
    return c, [g]


def _draw(seed):
    if seed_class(seed) == "refused":
        return _refused_case(seed)
    c = _draw_module(seed)
    rng = c["rng"]
    kinds = ["seams", "least", "tight", "thin"] + (["seams"] if rng.random() < 0.5 else [])
    return c, [_draw_geometry(rng, c, k) for k in kinds]


def gen_chain_case(seed):
    """-> (module text on the first geometry, meta)"""
    c, geoms = _draw(seed)
    form, rank, elem, radii, nin = c["form"], c["rank"], c["elem"], c["radii"], c["nin"]
    entries = {}
    for ns in _ns_list(c):
        w = window(form, rank, radii, nin, ns)
        gc = geom_consts(elem, radii, ns)
        entries[ns] = None if w is None else dict(window=w, MK=gc["MK"], KEEPK=gc["KEEPK"], WARM=gc["WARM"],
                                                  KEEPJ=keepj(form, rank, radii, nin, ns))
    for g in geoms:
        mask = _never_read(c, g)
        # the Euler step's rule outside the bounds is arithmetic (u + dt * u): it keeps finite data
        g["nan_cells"] = [int(m.sum()) for m in mask] if form != "euler" else [0] * nin
    g0 = geoms[0]
    meta = dict(seed=seed, form=form, rank=rank, elem=elem, radii=tuple(radii), offsets=list(c["offsets"]),
                one_sided=c["one_sided"], centre_only=c["ncen"], nin=nin, uses_index=c["uses_index"], uses_if=c["uses_if"],
                wide=max(radii) > 1, entries=entries, function="step" if form == "euler" else "op",
                oracle_function="step" if form == "euler" else "entry", geometries=geoms,
                module_of=REFUSED_BASE.get(seed, seed),
                leapfrog_capable=form == "leapfrog" and leapfrog_capable(rank, radii, nin))
    return module_text(c, g0["shape"], g0["origin"], g0["lb"], g0["ub"]), meta


def compile_text(seed):
    """the text a seed's module is compiled from: its own, or the module it borrows"""
    return gen_chain_case(REFUSED_BASE.get(seed, seed))[0]


def geometry_text(seed, gi):
    """the seed's module on geometry gi, for the oracle"""
    c, geoms = _draw(seed)
    g = geoms[gi]
    return module_text(c, g["shape"], g["origin"], g["lb"], g["ub"])


def inputs(seed, gi, nan=True):
    """the inputs of geometry gi in entry order -- chain / euler: (u, c...); leapfrog: (u, u_prev, c...) -- and the never-read
    masks.  0.01 x hashed values with -0 and +0 sprinkled in; coefficient fields 0.5 + 0.25 x hash; NaN on the never-read
    cells in the chain and leapfrog forms"""
    import helpers
    c, geoms = _draw(seed)
    g = geoms[gi]
    dt = np.float64 if c["elem"] == "f64" else np.float32
    shape = tuple(g["shape"])
    nstate = 2 if c["form"] == "leapfrog" else 1
    out = []
    for k in range(c["nin"]):
        h = helpers.hash_field(shape, dt, seed=1000 * (seed % 997) + 37 * k + 5 + gi)
        if k < nstate:
            a = (h * dt(0.01)).astype(dt)
            flat = a.reshape(-1)
            flat[::7] = -0.0
            flat[3::11] = 0.0
        else:
            a = (dt(0.5) + dt(0.25) * h).astype(dt)
        out.append(a)
    masks = _never_read(c, g)
    if nan and c["form"] != "euler":
        for a, m in zip(out, masks):
            a[m] = np.nan
    return out, masks


def oracle_states(seed, gi, steps, nan=True):
    """the oracle stepped call by call: -> [state after 0, 1, .. steps applies] (chain / euler), or the same list for the
    leapfrog with the rotation done here (state n+1 = @entry(state n, state n-1, c...); state -1 is input 1)"""
    import helpers
    c, geoms = _draw(seed)
    m = helpers.oracle.Module.parse(geometry_text(seed, gi))
    ins, _ = inputs(seed, gi, nan)
    fn = "step" if c["form"] == "euler" else "entry"
    states = [ins[0]]
    if c["form"] == "leapfrog":
        prev, extra = ins[1], ins[2:]
        for _ in range(steps):
            nxt = np.full_like(states[-1], SENTINEL)
            m.call(fn, nxt, states[-1], prev, *extra)
            prev = states[-1]
            states.append(nxt)
    else:
        for _ in range(steps):
            nxt = np.full_like(states[-1], SENTINEL)
            m.call(fn, nxt, states[-1], *ins[1:])
            states.append(nxt)
    return states
