"""Seeded applies of rank 4 to 6 for both lowering paths beyond rank 3 (no GPU needed to generate or lower them).

An apply of rank R = 4..6 has L = R - 3 leading (batch / component) dimensions.  Without offsets along them the host
peels them off and launches one rank-3 apply per leading index (lowered_runtime.hpp run_apply_batched: "peeled"); with
an offset along a leading dimension the rank-generic kernel runs (kernels/apply_nd.hpp: "nd").  Every module here has
one opdef of each kind, so both paths run in every rank, and an @entry that composes them.

What a case varies, and what a wrong kernel or host loop would get wrong on it:
  - a result box with a random logical origin, leading extents of 1 to 6 (a wrong leading origin or extent);
  - ragged or aligned rows (the vector tail);
  - inputs 1.. in boxes of their own that contain the result's, with margins along leading and trailing dimensions (the
    per-input sub-buffer offset of the peeled launch, the per-input shift and clamp of the nd kernel); input 0 keeps
    the result's box, which the copy-through requires;
  - apply.bounds that are the full box, cut into leading and trailing dimensions, or empty along exactly one leading
    dimension (the zero-trip launches of the peeled path, the copy-through of the nd kernel);
  - bodies that read the index arguments of every leading dimension and of one trailing dimension, so that a wrong
    leading index mapping changes bits.

Which path an apply takes is read from the emitted source (paths()), never restated here; the generator only states
what it meant, and tests/test_nd_cases.py checks that the two agree."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

CONSTS = [0.5, -0.25, 1.5, 0.125, -0.75, 2.0, -1.25, 0.375, 3.0, -0.0625, 1.75, 0.3125]   # test_fuzz_gpu.CONSTS
VK = {"f64": 2, "f32": 4}                                                                # cells per 16-byte vector

Box = Tuple[Tuple[int, ...], Tuple[int, ...]]


@dataclass
class OpSpec:
    name: str
    kind: str                         # what the generator meant: "peeled" or "nd"
    nin: int
    bounds: Box
    bounds_mode: str                  # "full", "cut" or "empty-lead"
    accesses: List[Tuple[int, Tuple[int, ...]]]
    lines: list                       # body: strings and ("access", var, input, offsets) items
    lead_index_dims: Tuple[int, ...]  # leading dimensions whose index argument the body reads


@dataclass
class Case:
    seed: int
    rank: int
    elem: str
    boxes: List[Box]                  # boxes[0]: the result's (and input 0's); boxes[k]: input k's own box
    ops: List[OpSpec]
    store: Optional[Box]              # @entry stores the composed result to this sub-box (None: the whole field)
    text: str = field(repr=False, default="")

    @property
    def lead(self) -> int:
        return self.rank - 3

    @property
    def shape(self) -> Tuple[int, ...]:
        return box_shape(self.boxes[0])

    def in_shape(self, k: int) -> Tuple[int, ...]:
        return box_shape(self.boxes[k])

    @property
    def dtype(self):
        return np.float64 if self.elem == "f64" else np.float32

    @property
    def nmax(self) -> int:
        return max(o.nin for o in self.ops)

    @property
    def ragged(self) -> bool:
        return self.shape[-1] % VK[self.elem] != 0


def box_shape(b: Box) -> Tuple[int, ...]:
    return tuple(u - l for l, u in zip(*b))


def _battr(b: Box) -> str:
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, b[0]))}], ub = [{', '.join(map(str, b[1]))}]>"


def _types(elem: str, boxes: List[Box]) -> List[str]:
    L = ['#l = #neptune_ir.location<"cell">']
    for k, b in enumerate(boxes):
        L += [f"#b{k} = {_battr(b)}", f"!t{k} = !neptune_ir.temp<element = {elem}, bounds = #b{k}, location = #l>",
              f"!f{k} = !neptune_ir.field<element = {elem}, bounds = #b{k}, location = #l>"]
    return L


def opdef_text(op: OpSpec, elem: str, rank: int, lead_consts: Optional[Tuple[int, ...]] = None, name: Optional[str] = None):
    """the opdef of `op`.  lead_consts: the same body as a rank-3 opdef at one fixed leading index -- the leading index
    arguments become constants, every access and the bounds keep their last three components (types !t0.. must then
    be declared with the last three components of the boxes)"""
    L = 0 if lead_consts is None else rank - 3
    tys = ", ".join(f"!t{k}" for k in range(op.nin))
    bnd = (op.bounds[0][L:], op.bounds[1][L:])
    idx = ", ".join(f"%i{d}: index" for d in range(L, rank))
    ins = ", ".join(f"%in{k}: !t{k}" for k in range(op.nin))
    body = [f"%i{d} = arith.constant {c} : index" for d, c in enumerate(lead_consts or ())]
    for item in op.lines:
        if isinstance(item, tuple):
            _, var, k, off = item
            body.append(f"{var} = neptune_ir.access %in{k}[{', '.join(map(str, off[L:]))}] : !t{k} -> {elem}")
        else:
            body.append(item)
    text = [f"  neptune_ir.nonlinear_opdef @{name or op.name} : ({tys}) -> !t0 {{",
            "  ^bb0(" + ", ".join(f"%u{k}: !t{k}" for k in range(op.nin)) + "):",
            "    %r = neptune_ir.apply(" + ", ".join(f"%u{k}" for k in range(op.nin)) + f") attributes {{bounds = {_battr(bnd)}}} : "
            f"({tys}) -> !t0 {{", f"      ^bb0({idx}, {ins}):"] + ["        " + s for s in body] + \
           ["    }", "    neptune_ir.return %r : !t0", "  }"]
    return "\n".join(text)


def slice_module(case: Case, op: OpSpec, lead_index: Tuple[int, ...]) -> str:
    """a rank-3 module whose @op is `op` at the fixed leading index `lead_index` (logical), on the rank-3 slices of its
    inputs"""
    L = case.lead
    boxes3 = [(b[0][L:], b[1][L:]) for b in case.boxes[:op.nin]]
    return "\n".join(_types(case.elem, boxes3) + ["module {", opdef_text(op, case.elem, case.rank, lead_index, "op"), "}"]) + "\n"


def lead_slice(case: Case, k: int, lead_index: Tuple[int, ...]) -> Tuple[int, ...]:
    """the physical leading index of input k's rank-3 slice at logical leading index `lead_index`"""
    return tuple(j - lb for j, lb in zip(lead_index, case.boxes[k][0][:case.lead]))


def _gen_op(rng, name, kind, rank, elem, boxes, nin, out_box):
    L = rank - 3
    shape = box_shape(out_box)
    lb0, ub0 = out_box
    # apply.bounds: the full box, or cut into the trailing (and where the extent allows, the leading) dimensions
    mode = str(rng.choice(["full", "cut", "cut", "empty-lead"]))
    radius = int(rng.choice([1, 1, 2]))
    blb, bub = list(lb0), list(ub0)
    if mode != "full":
        for d in range(rank):
            if d < L:
                if shape[d] >= 3 and rng.random() < 0.7:
                    blb[d] += int(rng.integers(0, 2))
                    bub[d] -= int(rng.integers(1, 2))
            else:
                blb[d] += min(radius + int(rng.integers(0, 2)), (shape[d] - 1) // 2)   # never empty here
                bub[d] -= min(radius + int(rng.integers(0, 2)), (shape[d] - 1) // 2)
    if kind == "nd" and nin == 1 and not any(blb[d] > lb0[d] and bub[d] < ub0[d] for d in range(L)):
        d = max(range(L), key=lambda e: shape[e])          # input 0 alone: a leading cut makes room for its offset
        assert shape[d] >= 3, "the caller gives the nd opdef a second input"
        blb[d], bub[d] = lb0[d] + 1, ub0[d] - 1
        mode = "cut" if mode == "full" else mode
    nominal = (tuple(blb), tuple(bub))

    def valid(k, off):          # every cell of the nominal bounds reads inside input k's box
        ib = boxes[k]
        return all(nominal[0][d] + off[d] >= ib[0][d] and nominal[1][d] - 1 + off[d] < ib[1][d] for d in range(rank))
    box_fp = radius == 1 and rng.random() < 0.35           # box footprints of radius 1, stars up to 2 (as test_fuzz_gpu)
    accesses = []
    for k in range(nin):
        accesses.append((k, (0,) * rank))
        if k > 0 and rng.random() < 0.3:
            continue
        for _ in range(int(rng.integers(2, 7))):
            if box_fp:
                off = [0] * L + [int(rng.integers(-radius, radius + 1)) for _ in range(3)]
            else:
                d = int(rng.integers(L, rank))
                off = [int(rng.choice([-radius, -1, 1, radius])) if a == d else 0 for a in range(rank)]
            if kind == "nd" and rng.random() < 0.5:
                off[int(rng.integers(0, L))] = int(rng.choice([-1, 1]))
            off = tuple(off)
            if any(off) and valid(k, off) and (k, off) not in accesses:
                accesses.append((k, off))
    if kind == "nd" and not any(any(off[:L]) for _, off in accesses):
        cand = [(k, tuple(s if a == d else 0 for a in range(rank))) for k in range(nin) for d in range(L) for s in (-1, 1)]
        cand = [c for c in cand if valid(*c)]
        assert cand, "no leading offset fits: the caller gives input 1 a leading margin"
        accesses.append(cand[int(rng.integers(0, len(cand)))])
    if mode == "empty-lead":
        d = int(rng.integers(0, L))
        p = int(rng.integers(lb0[d], ub0[d] + 1))
        blb[d], bub[d] = p, p
    lines: list = []
    vals = []
    for n, (k, off) in enumerate(accesses):
        lines.append(("access", f"%a{n}", k, off))
        vals.append(f"%a{n}")
    cnt = 0

    def const():
        nonlocal cnt
        cnt += 1
        lines.append(f"%c{cnt} = arith.constant {CONSTS[int(rng.integers(0, len(CONSTS)))]!r} : {elem}")
        return f"%c{cnt}"

    def binop(a, b):
        nonlocal cnt
        cnt += 1
        op = rng.choice(["arith.addf", "arith.subf", "arith.mulf", "arith.addf", "arith.subf", "arith.maximumf", "arith.minimumf"])
        lines.append(f"%v{cnt} = {op} {a}, {b} : {elem}")
        return f"%v{cnt}"

    def index_term(d):              # CONST * float(i_d)
        nonlocal cnt
        cnt += 1
        w = cnt
        lines.append(f"%w{w} = arith.index_cast %i{d} : index to i64")
        lines.append(f"%wf{w} = arith.sitofp %w{w} : i64 to {elem}")
        c = const()
        cnt += 1
        lines.append(f"%v{cnt} = arith.mulf {c}, %wf{w} : {elem}")
        return f"%v{cnt}"
    acc = vals[0]
    for v in vals[1:]:
        term = v
        if rng.random() < 0.6:
            c = const()
            cnt += 1
            term = f"%v{cnt}"
            lines.append(f"{term} = arith.mulf {c}, {v} : {elem}")
        acc = binop(acc, term)
    if rng.random() < 0.4:
        cnt += 1
        lines.append(f"%v{cnt} = math.absf {acc} : {elem}")
        acc = binop(f"%v{cnt}", vals[0])
    if rng.random() < 0.4:
        c = const()
        cnt += 1
        lines.append(f"%v{cnt} = arith.divf {acc}, {c} : {elem}")
        acc = f"%v{cnt}"
    if rng.random() < 0.25:                     # sqrt(|x|): IEEE-exact on both sides
        cnt += 1
        lines.append(f"%g{cnt} = math.absf {acc} : {elem}")
        lines.append(f"%v{cnt} = math.sqrt %g{cnt} : {elem}")
        acc = f"%v{cnt}"
    if rng.random() < 0.4:                      # select on a float compare
        z = const()
        cnt += 1
        lines.append(f"%p{cnt} = arith.cmpf {rng.choice(['olt', 'oge', 'une', 'ogt'])}, {vals[0]}, {z} : {elem}")
        lines.append(f"%v{cnt} = arith.select %p{cnt}, {acc}, {vals[-1]} : {elem}")
        acc = f"%v{cnt}"
    # every leading index argument, and one trailing one, so that a wrong leading index or origin changes bits
    tdim = int(rng.integers(L, rank))
    for d in list(range(L)) + [tdim]:
        acc = binop(acc, index_term(d))
    if rng.random() < 0.5:                      # scf.if on a leading index argument
        d = int(rng.integers(0, L))
        thr = lb0[d] + shape[d] // 2
        cnt += 1
        lines.append(f"%thr{cnt} = arith.constant {thr} : index")
        lines.append(f"%q{cnt} = arith.cmpi slt, %i{d}, %thr{cnt} : index")
        lines.append(f"%v{cnt} = scf.if %q{cnt} -> ({elem}) {{")
        lines.append(f"  %cb{cnt} = arith.mulf {acc}, {vals[0]} : {elem}")
        lines.append(f"  scf.yield %cb{cnt} : {elem}")
        lines.append("} else {")
        lines.append(f"  %cc{cnt} = arith.subf {acc}, {vals[-1]} : {elem}")
        lines.append(f"  scf.yield %cc{cnt} : {elem}")
        lines.append("}")
        acc = f"%v{cnt}"
    lines.append(f"neptune_ir.yield {acc} : {elem}")
    return OpSpec(name, kind, nin, (tuple(blb), tuple(bub)), mode, accesses, lines, tuple(range(L)))


def gen_case(seed: int) -> Case:
    """one module: a result box of rank 4, 5 or 6 (rank and element type rotate with the seed), inputs in boxes of their
    own, a peeled and an nd opdef in random order, and @entry(out, in0, ...) = store(op_b(op_a(in0, ...), in1, ...))"""
    rng = np.random.default_rng(seed)
    rank = 4 + seed % 3
    elem = ("f64", "f32")[(seed // 3) % 2]
    L = rank - 3
    while True:
        lead = [int(rng.choice([1, 1, 2, 3, 5, 6])) for _ in range(L)]
        if int(np.prod(lead)) <= 30:
            break
    vk = VK[elem]
    last = int(rng.choice([128, 192, 256])) * (vk // 2) + (int(rng.integers(1, vk)) if rng.random() < 0.5 else 0)
    shape = lead + [int(rng.integers(5, 10)), int(rng.integers(5, 10)), last]
    origin = [int(rng.integers(-3, 5)) for _ in range(rank)]
    out_box = (tuple(origin), tuple(o + n for o, n in zip(origin, shape)))
    nmax = int(rng.integers(1, 5))
    kinds = ["peeled", "nd"] if rng.random() < 0.5 else ["nd", "peeled"]
    nins = [int(rng.integers(1, nmax + 1)) for _ in kinds]
    nins[int(rng.integers(0, 2))] = nmax
    if nins[kinds.index("nd")] < 2 and min(lead) < 3:      # no room for a leading offset on input 0: give input 1 one
        nmax = max(nmax, 2)
        nins[kinds.index("nd")] = 2
    boxes = [out_box]
    for k in range(1, nmax):
        lo = [int(rng.integers(0, 3)) for _ in range(L)] + [int(rng.integers(0, 4)) for _ in range(3)]
        hi = [int(rng.integers(0, 3)) for _ in range(L)] + [int(rng.integers(0, 4)) for _ in range(3)]
        if k == 1:                                           # input 1 has room for a leading offset somewhere
            d = int(rng.integers(0, L))
            lo[d], hi[d] = max(lo[d], 1), max(hi[d], 1)
        boxes.append((tuple(a - g for a, g in zip(out_box[0], lo)), tuple(a + g for a, g in zip(out_box[1], hi))))
    ops = [_gen_op(rng, f"op{n}", kind, rank, elem, boxes, nin, out_box) for n, (kind, nin) in enumerate(zip(kinds, nins))]
    store = None
    if rng.random() < 0.5:
        store = (tuple(o + int(rng.integers(0, 2 if n > 1 else 1)) for o, n in zip(out_box[0], shape)),
                 tuple(u - int(rng.integers(0, 2 if n > 2 else 1)) for u, n in zip(out_box[1], shape)))
    case = Case(seed, rank, elem, boxes, ops, store)
    case.text = module_text(case)
    return case


def module_text(case: Case) -> str:
    rank, elem = case.rank, case.elem
    mr = "x".join("?" * rank) + "x" + elem
    head = _types(elem, case.boxes) + ["module {"]
    for op in case.ops:
        head.append(opdef_text(op, elem, rank))
    a, b = case.ops
    E = [f"  func.func @entry(%out: memref<{mr}>, " + ", ".join(f"%m{k}: memref<{mr}>" for k in range(case.nmax)) + f") -> memref<{mr}> {{",
         f"    %fo = neptune_ir.wrap %out : memref<{mr}> -> !f0"]
    for k in range(case.nmax):
        E.append(f"    %f{k} = neptune_ir.wrap %m{k} : memref<{mr}> -> !f{k}")
        E.append(f"    %t{k} = neptune_ir.load %f{k} : !f{k} -> !t{k}")
    tys = lambda n: "(" + ", ".join(f"!t{k}" for k in range(n)) + ")"   # noqa: E731
    E.append(f"    %y0 = neptune_ir.apply_nonlinear @{a.name}(" + ", ".join(f"%t{k}" for k in range(a.nin)) + f") : {tys(a.nin)} -> !t0")
    E.append(f"    %y1 = neptune_ir.apply_nonlinear @{b.name}(" + ", ".join(["%y0"] + [f"%t{k}" for k in range(1, b.nin)])
             + f") : {tys(b.nin)} -> !t0")
    if case.store is None:
        E.append("    neptune_ir.store %y1 to %fo : !t0 to !f0")
    else:
        E.append(f"    neptune_ir.store %y1 to %fo {{bounds = {_battr(case.store)}}} : !t0 to !f0")
    E += [f"    %res = neptune_ir.unwrap %fo : !f0 -> memref<{mr}>", f"    func.return %res : memref<{mr}>", "  }"]
    head.append("\n".join(E))
    head.append("}")
    return "\n".join(head) + "\n"


def tiles_apply(case: Case) -> bool:
    """can a forced march tile take every peeled launch?  The sub-slab of leading index j starts j * (cells per rank-3 slab)
    cells into input 0 and the result; the march kernel wants those starts on 16-byte boundaries and refuses a forced tile
    otherwise (apply_launch.hpp plan_apply), while the automatic choice falls back to the direct kernel for that index"""
    return int(np.prod(case.shape[-3:])) * np.dtype(case.dtype).itemsize % 16 == 0


def paths(text: str) -> Dict[str, str]:
    """opdef name -> "peeled" / "nd", as the lowering emitted it"""
    from neptune_hip import lowering
    src, rep = lowering.to_hip(text)
    out = {}
    for a in rep["applies"]:
        name = a["function"]
        peeled = f"nl::run_apply_batched<Body_{name}_0, " in src
        nd = f"nl::run_apply_nd<Body_{name}_0, " in src
        assert peeled != nd, name
        out[name] = "peeled" if peeled else "nd"
    return out


def lead_indices(case: Case):
    """every logical leading multi-index of the result box, row-major"""
    lb = case.boxes[0][0][:case.lead]
    return [tuple(int(a + j) for a, j in zip(lb, idx)) for idx in np.ndindex(*case.shape[:case.lead])]


def inside_lead(op: OpSpec, lead_index) -> bool:
    return all(lb <= j < ub for j, lb, ub in zip(lead_index, op.bounds[0], op.bounds[1]))


def features(case: Case) -> set:
    """the coverage marks of one case (test_nd_cases.py checks the seed list against its quotas)"""
    L, shape = case.lead, case.shape
    f = {f"rank{case.rank}", case.elem, f"rank{case.rank}-{case.elem}", "ragged" if case.ragged else "aligned", "store-box" if case.store else "store-full"}
    f.add("tiles" if tiles_apply(case) else "slab-misaligned")
    if case.ragged and tiles_apply(case):
        f.add("tiles-ragged")
    if 1 in shape[:L]:
        f.add("lead-extent-1")
        if max(shape[:L]) >= 5:
            f.add("lead-extent-1-beside-5")
    for op in case.ops:
        f |= {op.kind, f"{op.kind}-rank{case.rank}", f"{op.kind}-{op.bounds_mode}", f"nin{op.nin}"}
        f |= {f"{op.kind}-lead-index-{d}" for d in op.lead_index_dims}
        ins = [j for j in lead_indices(case) if inside_lead(op, j)]
        if op.bounds_mode == "cut" and 0 < len(ins) < len(lead_indices(case)):
            f.add(f"{op.kind}-lead-cut")
        for k in range(1, op.nin):
            lo, hi = case.boxes[k][0][:L], case.boxes[k][1][:L]
            if any(a < b for a, b in zip(lo, case.boxes[0][0])):
                f.add(f"{op.kind}-lead-margin")
            if any(a < b or c > e for a, b, c, e in zip(lo[1:], case.boxes[0][0][1:L], hi[1:], case.boxes[0][1][1:L])):
                f.add(f"{op.kind}-inner-lead-margin")     # the input's leading extents enter the sub-buffer offset
    return f


# The seeds the GPU tests run: every rank, both element types, both paths in every module.  test_nd_cases.py checks that
# they meet the coverage quotas of the issue; a seed is replaced only together with that check.
SEEDS = list(range(14))


# ---- one rank-4 f32 field per path beyond 2^31 cells (test_nd_fuzz_gpu.py).  The input is affine in the logical index with
# integer coefficients, so every value, partial sum and product of the body is an integer below 2^24 and exact in f32.  The
# body is a Laplacian (star along the last three dimensions for the peeled path, along all four for nd) plus (u - that
# affine function): exactly 0 on every cell inside the bounds unless a launch reads another sub-slab, another cell or the
# wrong index argument; every other cell is input 0's.
LARGE_SHAPE = (3, 1024, 1024, 704)
LARGE_LB = (-1, 2, -3, 5)
LARGE_COEF = (3, 5, 7, 11)
LARGE_COEF0 = -20000


def large_bounds(path, shape=LARGE_SHAPE):
    lb = [a + 1 for a in LARGE_LB]
    ub = [a + n - 1 for a, n in zip(LARGE_LB, shape)]
    if path == "peeled":                      # every leading index computes
        lb[0], ub[0] = LARGE_LB[0], LARGE_LB[0] + shape[0]
    return lb, ub


def large_affine(shape):
    """numpy: LARGE_COEF0 + sum_d LARGE_COEF[d] * (logical index d), f32"""
    idx = [np.arange(n, dtype=np.int64) + o for n, o in zip(shape, LARGE_LB)]
    v = LARGE_COEF0 + sum(c * i.reshape([-1 if e == d else 1 for e in range(4)]) for d, (c, i) in enumerate(zip(LARGE_COEF, idx)))
    return np.broadcast_to(v, shape).astype(np.float32)


def large_text(path, shape=LARGE_SHAPE):
    offs = [tuple(s if a == d else 0 for a in range(4)) for d in range(0 if path == "nd" else 1, 4) for s in (-1, 1)]
    lb, ub = large_bounds(path, shape)
    L = [f"%a{n} = neptune_ir.access %u[{', '.join(map(str, o))}] : !t -> f32" for n, o in enumerate(offs)]
    L += ["%c = neptune_ir.access %u[0, 0, 0, 0] : !t -> f32", "%s0 = arith.addf %a0, %a1 : f32"]
    L += [f"%s{n - 1} = arith.addf %s{n - 2}, %a{n} : f32" for n in range(2, len(offs))]
    L += [f"%k = arith.constant {float(len(offs))!r} : f32", "%kc = arith.mulf %k, %c : f32",
          f"%lap = arith.subf %s{len(offs) - 2}, %kc : f32", f"%e = arith.constant {float(LARGE_COEF0)!r} : f32"]
    acc = "%e"
    for d in range(4):
        L += [f"%w{d} = arith.index_cast %i{d} : index to i64", f"%wf{d} = arith.sitofp %w{d} : i64 to f32",
              f"%k{d} = arith.constant {float(LARGE_COEF[d])!r} : f32", f"%m{d} = arith.mulf %k{d}, %wf{d} : f32",
              f"%f{d} = arith.addf {acc}, %m{d} : f32"]
        acc = f"%f{d}"
    L += [f"%dev = arith.subf %c, {acc} : f32", "%o = arith.addf %lap, %dev : f32", "neptune_ir.yield %o : f32"]
    box = (LARGE_LB, tuple(a + n for a, n in zip(LARGE_LB, shape)))
    mr = "memref<?x?x?x?xf32>"
    return "\n".join([
        '#l = #neptune_ir.location<"cell">', f"#b = {_battr(box)}",
        "!t = !neptune_ir.temp<element = f32, bounds = #b, location = #l>",
        "!f = !neptune_ir.field<element = f32, bounds = #b, location = #l>", "module {",
        "  neptune_ir.nonlinear_opdef @lap : (!t) -> !t {", "  ^bb0(%v: !t):",
        f"    %r = neptune_ir.apply(%v) attributes {{bounds = {_battr((lb, ub))}}} : (!t) -> !t {{",
        "      ^bb0(%i0: index, %i1: index, %i2: index, %i3: index, %u: !t):"] + ["        " + s for s in L] + [
        "    }", "    neptune_ir.return %r : !t", "  }",
        f"  func.func @entry(%out: {mr}, %in: {mr}) -> {mr} {{", f"    %fo = neptune_ir.wrap %out : {mr} -> !f",
        f"    %fi = neptune_ir.wrap %in : {mr} -> !f", "    %t = neptune_ir.load %fi : !f -> !t",
        "    %y = neptune_ir.apply_nonlinear @lap(%t) : (!t) -> !t", "    neptune_ir.store %y to %fo : !t to !f",
        f"    %res = neptune_ir.unwrap %fo : !f -> {mr}", f"    func.return %res : {mr}", "  }", "}"]) + "\n"
