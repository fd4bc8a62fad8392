"""Seeded random GROUPS of sibling applies, as module texts -- no GPU needed.  One module is one
@entry(out_0 .. out_{M-1}, in_0 .. in_{F-1}): every input loaded once, M consecutive applies with the same apply.bounds over
subsets of the F inputs (each member lists its own unknown first, in an order of its own), one store per member.  What the
two hand-written system fixtures do not have is drawn here: subset input maps, a copy-through source that is not the
member's index, footprints that differ between the members (so that the union ring the kernel holds is wider than a
member's own reach), asymmetric footprints, index arguments and scf.if in some members only, a box origin away from 0,
rows around the lane-vector / wave / workgroup boundaries, zero-trip and whole-box apply.bounds, and the three kinds of
store (forwardable, sub-box, a result with a second reader).  Only IEEE-exact operations, never a division by a field value.

gen_group_module(seed) -> (text, shape, origin, elem, n_members, n_fields, meta); `meta` records what the seed drew, and
tests/test_group_fuzz_host.py makes the coverage over SEEDS binding.  The class of a seed is seed // 1000 (CLASSES)."""
import numpy as np

from test_fuzz_gpu import CONSTS, gen_chain

# seed // 1000 -> class.  "random": everything drawn within what has a fused march form.  The forced classes pin the other
# launch forms and the two degenerate apply.bounds.
CLASSES = {0: "random", 1: "direct", 2: "members2", 3: "members3", 4: "zero_trip", 5: "full_box"}
KERNEL_OF = {"random": "march", "direct": "direct", "members2": "members", "members3": "members", "zero_trip": "march",
             "full_box": "march"}

# 24 modules, 6 of rank 3 (the slow compiles).  tests/test_group_fuzz_host.py asserts what this list covers.
SEEDS = [0, 3, 6, 18, 21, 33, 1, 4, 7, 19, 25, 8, 14, 23, 35, 1000, 1005, 2000, 2003, 3002, 4001, 4002, 5000, 5003]
# the seeds of the aliasing test: a member's destination is its own input 0 / an input only other members read
ALIAS_SEEDS = [1, 3, 8, 1000, 2003]


def seed_class(seed):
    return CLASSES[seed // 1000]


def seed_rank_elem(seed):
    """rank and element type follow from the seed, so that a short list covers every pair"""
    cls, n = seed_class(seed), seed % 1000
    elem = "f64" if (n // 3) % 2 == 0 else "f32"
    if cls == "direct":
        return 1, ("f64" if n % 2 == 0 else "f32")
    if cls == "members2":
        return 2, ("f64" if n % 2 == 0 else "f32")
    if cls == "members3":
        return 3, ("f64" if n % 2 == 0 else "f32")
    if cls == "zero_trip":
        return 1 + n % 2, ("f32" if n % 2 == 0 else "f64")
    if cls == "full_box":
        return 2 + n % 2, ("f64" if n % 2 == 0 else "f32")
    return 1 + n % 3, elem


def _last_extent(rng, vk, need):
    """rows that straddle the lane-vector (vk cells), wave (64 lanes) and workgroup (up to 4 waves) boundaries, or shorter
    than one wave row; `need`: the least extent the footprint leaves a non-empty apply.bounds in"""
    span = vk * 64
    cands = [span * k + e for k in (1, 2, 4) for e in (-1, 0, 1)]
    cands.append(int(rng.integers(max(need, 5 * vk), span - 2 * vk)))       # shorter than a single wave row
    return int(cands[int(rng.integers(0, len(cands)))])


def _star_offsets(rng, rank, radius, n_off, sign):
    """offsets along one axis each; the first one reaches `radius`.  sign[d] in (-1, 0, 1): 0 both directions"""
    out = []
    for n in range(n_off):
        d = int(rng.integers(0, rank))
        a = radius if n == 0 else int(rng.choice([1, radius]))
        s = sign[d] if sign[d] else int(rng.choice([-1, 1]))
        off = tuple(s * a if x == d else 0 for x in range(rank))
        if off not in out:
            out.append(off)
    return out


def _box_offsets(rng, rank, radius, n_off, sign):
    """offsets anywhere in the (2 radius + 1)^rank window; the first one is a diagonal"""
    def comp(d, nonzero):
        lo, hi = (-radius if sign[d] <= 0 else 0), (radius if sign[d] >= 0 else 0)
        while True:
            v = int(rng.integers(lo, hi + 1))
            if v or not nonzero:
                return v
    out = []
    for n in range(n_off):
        off = tuple(comp(d, n == 0 and d >= rank - 2) for d in range(rank))
        if any(off) and off not in out:
            out.append(off)
    return out


def _draw(seed):
    """everything a seed draws, as a dict: the module's structure before it becomes text"""
    cls = seed_class(seed)
    rank, elem = seed_rank_elem(seed)
    rng = np.random.default_rng(100003 * seed + 17)
    vk = 2 if elem == "f64" else 4
    # ---- the group's shape: M members over F inputs, member m's own unknown is input through[m]
    M = int(rng.choice([2, 3, 3, 4]))
    F = int(rng.integers(max(M, 2), 5))
    if cls in ("direct", "members2", "members3"):
        M = int(rng.choice([2, 3]))
        F = int(rng.integers(M, 5))
    perm = [int(x) for x in rng.permutation(F)]
    through = perm[:M]                                  # distinct: two members never advance the same field
    spare = perm[M:]                                    # nobody's unknown
    members = []                                        # per member: the fields it reads, its own first
    for m in range(M):
        others = [k for k in range(F) if k != through[m]]
        n_other = int(rng.integers(0, len(others) + 1))
        pick = [others[int(i)] for i in rng.permutation(len(others))[:n_other]]
        members.append([through[m]] + pick)
    # a field only ONE member reads that is nobody's unknown (a fixed input), in some seeds; every other spare field is
    # read by two members at least
    fixed = None
    if spare and rng.random() < 0.6:
        fixed = spare[0]
        reader = int(rng.integers(0, M))
        for m in range(M):
            if fixed in members[m] and m != reader:
                members[m].remove(fixed)
        if fixed not in members[reader]:
            members[reader].append(fixed)
    for k in range(F):                                  # every field is read; spares (not the fixed one) twice
        want = 2 if (k in spare and k != fixed) else 1
        while sum(k in mem for mem in members) < want:
            m = int(rng.integers(0, M))
            if k not in members[m]:
                members[m].append(k)
    if not any(sum(k in mem for mem in members) >= 2 for k in range(F)):      # one shared value: find_group needs it
        members[1].append(through[0])
    if cls in ("direct", "members2", "members3"):       # every member reads member 0's unknown: the field they differ on
        for mem in members[1:]:
            if through[0] not in mem:
                mem.append(through[0])
    # ---- footprints
    if cls == "full_box":
        mode = "centre"
    elif cls == "direct":
        mode = "beyond"                                 # rank 1, every member beyond the march kernel's 2 vk cells
    elif cls == "members2":
        mode = "box+r2"                                 # rank 2: a box member and a radius-2 star member
    elif cls == "members3":
        mode = "r2"                                     # rank 3: radius-2 stars
    elif rank == 3:
        mode = str(rng.choice(["star", "box", "star+box", "star+box"]))
    elif rank == 2:
        mode = str(rng.choice(["star", "mixed", "mixed", "box", "star+box", "star+box"]))
    else:
        mode = str(rng.choice(["star", "mixed", "mixed", "wide"]))
    # which fields may be read at offsets at all (the union's halo inputs): two in 3-D, one for wide 1-D stars
    max_halo = {3: 2, 2: 4, 1: 4}[rank]
    if mode in ("wide", "beyond"):
        max_halo = 1
    shared = [k for k in range(F) if sum(k in mem for mem in members) >= 2]
    halo = [shared[int(rng.integers(0, len(shared)))]]                        # a shared one first: that is where members differ
    if cls in ("direct", "members2", "members3"):
        halo = [through[0]]
    for k in (int(i) for i in rng.permutation(F)):
        if len(halo) < max_halo and k not in halo and rng.random() < 0.7:
            halo.append(k)
    asym = cls != "full_box" and rng.random() < 0.4
    sign = [0] * rank
    if asym:
        sign[int(rng.integers(0, rank))] = int(rng.choice([-1, 1]))
    acc, fp = [], []                                    # per member: [(member input, offset)], its footprint record
    for m in range(M):
        if mode in ("star", "centre"):
            style, radius = "star", 1
        elif mode == "box":
            style, radius = "box", 1
        elif mode == "star+box":
            style, radius = ("box" if m % 2 == int(seed % 2) else "star"), 1
        elif mode == "mixed":
            style, radius = "star", (2 if m % 2 == int(seed % 2) else 1)
        elif mode == "wide":
            style, radius = "star", int(rng.integers(3, 2 * vk + 1))
        elif mode == "beyond":
            style, radius = "star", 2 * vk + 1 + int(rng.integers(0, 2))
        elif mode == "box+r2":
            style, radius = ("box", 1) if m == 0 else ("star", 2 if m == 1 else int(rng.choice([1, 2])))
        else:                                           # "r2"
            style, radius = "star", (2 if m == 0 else int(rng.choice([1, 2])))
        a = []
        reach = {}
        for k, field in enumerate(members[m]):
            a.append((k, (0,) * rank))
            wants = mode != "centre" and field in halo and (rng.random() < 0.7 or (mode in ("beyond", "box+r2", "r2") and field == halo[0]))
            if not wants:
                reach.setdefault(field, 0)
                continue
            n_off = int(rng.integers(2, 6))
            offs = (_box_offsets if style == "box" else _star_offsets)(rng, rank, radius, n_off, sign)
            a += [(k, o) for o in offs]
            reach[field] = max(max(abs(c) for c in o) for o in offs)
        fp.append({"style": style if any(reach.values()) else "centre", "reach": reach})
        acc.append(a)
    if mode != "centre" and not any(any(f["reach"].values()) for f in fp):    # one member at least reads neighbours
        k0 = next((k for k, field in enumerate(members[0]) if field in halo), None)
        if k0 is None:
            members[0].append(halo[0])
            k0 = len(members[0]) - 1
            acc[0].append((k0, (0,) * rank))
        offs = (_box_offsets if mode == "box" else _star_offsets)(rng, rank, 1, 3, sign)
        acc[0] += [(k0, o) for o in offs]
        fp[0] = {"style": "box" if mode == "box" else "star", "reach": dict(fp[0]["reach"], **{members[0][k0]: 1})}
    # a box member is one only if an offset of its own has two non-zero components
    for m in range(M):
        if fp[m]["style"] == "box" and not any(sum(1 for c in o if c) > 1 for _, o in acc[m]):
            fp[m]["style"] = "star"
    # ---- the box and apply.bounds: per side what the members reach, plus 0 or 1, unevenly
    lo = [max([0] + [-o[d] for a in acc for _, o in a]) for d in range(rank)]
    hi = [max([0] + [o[d] for a in acc for _, o in a]) for d in range(rank)]
    origin = [int(rng.integers(-3, 5)) for _ in range(rank)]
    shape = [int(rng.integers(max(5, lo[d] + hi[d] + 3), 14)) for d in range(rank - 1)]
    shape.append(_last_extent(rng, vk, lo[-1] + hi[-1] + 3))
    lb = [origin[d] + lo[d] + int(rng.integers(0, 2)) for d in range(rank)]
    ub = [origin[d] + shape[d] - hi[d] - int(rng.integers(0, 2)) for d in range(rank)]
    if cls == "full_box":
        lb, ub = list(origin), [o + n for o, n in zip(origin, shape)]
    if cls == "zero_trip":
        d = int(rng.integers(0, rank))
        ub[d] = lb[d]
    # ---- bodies: index arguments (scf.if with a conditional access, sitofp) in some members only
    uses_index = [bool(rng.random() < 0.5) for _ in range(M)]
    if rng.random() < 0.7 and len(set(uses_index)) == 1:
        uses_index[int(rng.integers(0, M))] ^= True
    bodies = []
    for m in range(M):
        L, vals = [], []
        for n, (k, off) in enumerate(acc[m]):
            L.append(f"%a{n} = neptune_ir.access %in{k}[{', '.join(map(str, off))}] : !t -> {elem}")
            vals.append(f"%a{n}")
        res, cnt = gen_chain(rng, L, vals, elem)
        if uses_index[m]:
            d = int(rng.integers(0, rank))
            thr = origin[d] + shape[d] // 2
            cnt += 1
            ck, coff = acc[m][-1] if rng.random() < 0.7 else acc[m][int(rng.integers(0, len(acc[m])))]
            L += [f"%thr{cnt} = arith.constant {thr} : index",
                  f"%q{cnt} = arith.cmpi slt, %i{d}, %thr{cnt} : index",
                  f"%v{cnt} = scf.if %q{cnt} -> ({elem}) {{",
                  f"  %ca{cnt} = neptune_ir.access %in{ck}[{', '.join(map(str, coff))}] : !t -> {elem}",
                  f"  %cb{cnt} = arith.addf {res}, %ca{cnt} : {elem}",
                  f"  scf.yield %cb{cnt} : {elem}",
                  "} else {",
                  f"  %w{cnt} = arith.index_cast %i{d} : index to i64",
                  f"  %wf{cnt} = arith.sitofp %w{cnt} : i64 to {elem}",
                  f"  %cc{cnt} = arith.subf {res}, %wf{cnt} : {elem}",
                  f"  scf.yield %cc{cnt} : {elem}",
                  "}"]
            res = f"%v{cnt}"
        L.append(f"neptune_ir.yield {res} : {elem}")
        bodies.append(L)
    # ---- stores: plain (forwardable), sub-box (never forwarded), or a result with a second reader
    stores, store_box = [], []
    for m in range(M):
        kind = str(rng.choice(["plain", "plain", "bounded", "twice"]))
        if cls in ("members3",) and kind == "twice":
            kind = "bounded"                            # (one apply less to compile in the slowest class)
        stores.append(kind)
        slb = [o + int(rng.integers(0, 3)) for o in origin]
        sub = [o + n - int(rng.integers(0, 3)) for o, n in zip(origin, shape)]
        store_box.append((slb, sub))
    trailing_first = bool(rng.random() < 0.5)           # the second readers right after the members, or after the stores
    return dict(seed=seed, cls=cls, rank=rank, elem=elem, M=M, F=F, through=through, members=members, fixed=fixed, mode=mode,
                halo=halo, asym=asym, acc=acc, fp=fp, origin=origin, shape=shape, lb=lb, ub=ub, uses_index=uses_index,
                bodies=bodies, stores=stores, store_box=store_box, trailing_first=trailing_first)


def _bounds(lb, ub):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, lb))}], ub = [{', '.join(map(str, ub))}]>"


def _text(c, only=None, plain=False):
    """the module of draw `c`; only = m: member m alone, as @entry(out, in_0 .. in_{F-1}); plain: every store a plain one and
    no second reader (the members' raw results)"""
    rank, elem, M, F = c["rank"], c["elem"], c["M"], c["F"]
    mr = "x".join("?" * rank) + "x" + elem
    which = list(range(M)) if only is None else [only]
    head = ['#l = #neptune_ir.location<"cell">', "#b = " + _bounds(c["origin"], [o + n for o, n in zip(c["origin"], c["shape"])]),
            "#bi = " + _bounds(c["lb"], c["ub"]),
            f"!t = !neptune_ir.temp<element = {elem}, bounds = #b, location = #l>",
            f"!f = !neptune_ir.field<element = {elem}, bounds = #b, location = #l>", "module {"]
    E = ["  func.func @entry(" + ", ".join([f"%out{m}: memref<{mr}>" for m in which] + [f"%m{k}: memref<{mr}>" for k in range(F)]) +
         f") -> memref<{mr}> {{"]
    for m in which:
        E.append(f"    %fo{m} = neptune_ir.wrap %out{m} : memref<{mr}> -> !f")
    for k in range(F):
        E.append(f"    %f{k} = neptune_ir.wrap %m{k} : memref<{mr}> -> !f")
        E.append(f"    %t{k} = neptune_ir.load %f{k} : !f -> !t")
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    for m in which:
        ins = c["members"][m]
        tys = ", ".join(["!t"] * len(ins))
        E.append(f"    %r{m} = neptune_ir.apply(" + ", ".join(f"%t{k}" for k in ins) + f") attributes {{bounds = #bi}} : ({tys}) -> !t {{")
        E.append(f"      ^bb0({idx}, " + ", ".join(f"%in{k}: !t" for k in range(len(ins))) + "):")
        E += ["        " + l for l in c["bodies"][m]]
        E.append("    }")
    twice = [] if plain else [m for m in which if c["stores"][m] == "twice"]

    def trailing():
        for m in twice:     # a single apply that reads member m's result: it must not join the group
            E.append(f"    %z{m} = neptune_ir.apply(%r{m}) attributes {{bounds = #bi}} : (!t) -> !t {{")
            E.append(f"      ^bb0({idx}, %in0: !t):")
            E.extend("        " + l for l in (f"%a0 = neptune_ir.access %in0[{', '.join(['0'] * rank)}] : !t -> {elem}",
                                              f"%c1 = arith.constant 0.5 : {elem}", f"%v1 = arith.mulf %c1, %a0 : {elem}",
                                              f"%v2 = arith.mulf %v1, %a0 : {elem}", f"%v3 = arith.subf %v2, %a0 : {elem}",
                                              f"neptune_ir.yield %v3 : {elem}"))
            E.append("    }")
    if c["trailing_first"]:
        trailing()
    for m in which:
        if c["stores"][m] == "bounded" and not plain:
            E.append(f"    neptune_ir.store %r{m} to %fo{m} {{bounds = {_bounds(*c['store_box'][m])}}} : !t to !f")
        else:
            E.append(f"    neptune_ir.store %r{m} to %fo{m} : !t to !f")
    if not c["trailing_first"]:
        trailing()
    for m in twice:
        E.append(f"    neptune_ir.store %z{m} to %fo{m} {{bounds = {_bounds(*c['store_box'][m])}}} : !t to !f")
    E += [f"    %res = neptune_ir.unwrap %fo{which[0]} : !f -> memref<{mr}>", f"    func.return %res : memref<{mr}>", "  }"]
    return "\n".join(head + ["\n".join(E), "}"]) + "\n"


def _meta(c):
    M, F = c["M"], c["F"]
    order = []                                          # the group's union inputs: fields in order of first use
    for mem in c["members"]:
        order += [k for k in mem if k not in order]
    maps = [[order.index(k) for k in mem] for mem in c["members"]]
    fp = c["fp"]
    halo_styles = {f["style"] for f in fp} - {"centre"}
    mixed = any(len({f["reach"][k] for f in fp if f["reach"].get(k, 0) > 0}) > 1 for k in range(F))
    centre_and_offsets = any(any(f["reach"].get(k, -1) == 0 for f in fp) and any(f["reach"].get(k, 0) > 0 for f in fp) for k in range(F))
    readers = [sum(k in mem for mem in c["members"]) for k in range(F)]
    # (b) of the aliasing test: member m, and a field that only OTHER members read
    foreign = [(m, k) for m in range(M) for k in range(F) if k not in c["members"][m] and readers[k] > 0]
    return {
        "class": c["cls"], "kernel": KERNEL_OF[c["cls"]], "rank": c["rank"], "elem": c["elem"], "members": M, "fields": F,
        "inputs": [f"%t{k}" for k in order], "field_of_input": order, "maps": maps, "through": [m[0] for m in maps],
        "member_fields": [list(mem) for mem in c["members"]],
        "subset_map": any(len(mem) < F for mem in c["members"]),
        "non_identity_through": [m[0] for m in maps] != list(range(M)),
        "fixed_input": c["fixed"] is not None, "mode": c["mode"],
        "star_plus_box": halo_styles == {"star", "box"}, "mixed_radius": mixed, "centre_and_offsets": centre_and_offsets,
        "asymmetric": bool(c["asym"]), "uses_index": list(c["uses_index"]),
        "zero_trip": any(a == b for a, b in zip(c["lb"], c["ub"])), "full_box": c["cls"] == "full_box",
        "stores": list(c["stores"]), "trailing_first": c["trailing_first"], "foreign": foreign,
        "lb": list(c["lb"]), "ub": list(c["ub"]), "store_box": [(list(a), list(b)) for a, b in c["store_box"]],
    }


def gen_group_module(seed):
    c = _draw(seed)
    return _text(c), tuple(c["shape"]), tuple(c["origin"]), c["elem"], c["M"], c["F"], _meta(c)


def member_module(seed, m):
    """member m of the seed's group cut out on its own: @entry(out, in_0 .. in_{F-1}) with that one apply, its store and --
    where its result has one -- its second reader"""
    return _text(_draw(seed), only=m)


def plain_module(seed):
    """the seed's group with a plain whole-field store per member and nothing after it: what @entry leaves in out_m is then
    member m's apply result itself (the oracle's view of what the group's geometry-level entry computes)"""
    return _text(_draw(seed), plain=True)


def inputs(seed, shape, elem, n_fields):
    import helpers
    dt = np.float64 if elem == "f64" else np.float32
    return [helpers.hash_field(shape, dt, seed=1000 * seed + 37 * k + 5) for k in range(n_fields)]
