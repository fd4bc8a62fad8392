"""Module texts and NumPy references for neptune_ir.reduce kinds max | min | l1 | l2 (no GPU needed).

The references restate DESIGN 3.3 in NumPy: max / min are arith.maximumf / minimumf folds (NaN if any cell is NaN,
-0 < +0; exact in any order), l1 and l2 are sums in the element type."""
import numpy as np

import reduce_cases as rc

KINDS = ("max", "min", "l1", "l2")
ALL_KINDS = ("sum",) + KINDS
OPTION = "// neptune-hip-option: reduce-kinds\n"


def _bnd(box):
    return rc._bnd(box)


def _mr(rank, elem):
    return "memref<" + "x".join("?" * rank) + "x" + elem + ">"


# ---- NumPy references -----------------------------------------------------------------------------------------------
def np_max(x):
    """arith.maximumf fold of the cells of x -> a scalar of x's dtype; -inf for no cells"""
    x = np.asarray(x).reshape(-1)
    dt = x.dtype.type
    if x.size == 0:
        return dt(-np.inf)
    if np.isnan(x).any():
        return dt(np.nan)
    m = x.max()
    if m == 0:   # -0 < +0: +0 if any cell is +0
        return dt(0.0) if (~np.signbit(x[x == 0])).any() else dt(-0.0)
    return dt(m)


def np_min(x):
    x = np.asarray(x).reshape(-1)
    dt = x.dtype.type
    if x.size == 0:
        return dt(np.inf)
    if np.isnan(x).any():
        return dt(np.nan)
    m = x.min()
    if m == 0:
        return dt(-0.0) if np.signbit(x[x == 0]).any() else dt(0.0)
    return dt(m)


def serial_sum(terms):
    """left-to-right sum in the terms' dtype, the order of the reference's loop"""
    terms = np.asarray(terms).reshape(-1)
    if terms.size == 0:
        return terms.dtype.type(0)
    return np.add.accumulate(terms, dtype=terms.dtype)[-1]   # accumulate is the serial loop, one rounding per step


def np_kind(kind, x):
    """the value of DESIGN 3.3 for the cells x, sums taken serially in x's dtype"""
    x = np.asarray(x)
    if kind == "max":
        return np_max(x)
    if kind == "min":
        return np_min(x)
    if kind == "sum":
        return serial_sum(x)
    if kind == "l1":
        return serial_sum(np.abs(x))
    assert kind == "l2"
    return np.sqrt(serial_sum(x * x))


# ---- plain reduces: every kind of one box in one module -------------------------------------------------------------
def plain_kinds_module(elem, box, reduce_boxes, kinds=ALL_KINDS, option=True):
    """@<kind>_<i>(a) -> elem for every kind and every reduce_boxes[i] (None: the whole field), rank 1..6"""
    rank = len(box[0])
    mr = _mr(rank, elem)
    funcs = []
    for i, red in enumerate(reduce_boxes):
        where = "" if red is None else f" in {_bnd(red)}"
        for kind in kinds:
            funcs.append(f"""  func.func @{kind}_{i}(%a: {mr}) -> {elem} {{
    %f = neptune_ir.wrap %a : {mr} -> !f
    %u = neptune_ir.load %f : !f -> !t
    %s = neptune_ir.reduce %u{where} {{kind = "{kind}"}} : !t -> {elem}
    func.return %s : {elem}
  }}
""")
    return f"""{OPTION if option else ""}#l = #neptune_ir.location<"cell">
!t = !neptune_ir.temp<element = {elem}, bounds = {_bnd(box)}, location = #l>
!f = !neptune_ir.field<element = {elem}, bounds = {_bnd(box)}, location = #l>
module {{
{"".join(funcs)}}}
"""


# ---- fused reduce(apply) --------------------------------------------------------------------------------------------
# bodies: text of the region's ops on %p0 (and %p1), yielding %y
def _residual_body(elem):
    """|A(u) - u| with A the 2-D 5-point average: reads input 0 at the centre and its four neighbours"""
    q = "0.25"
    return f"""        %c = neptune_ir.access %p0[0, 0] : !t -> {elem}
        %n = neptune_ir.access %p0[-1, 0] : !t -> {elem}
        %s = neptune_ir.access %p0[1, 0] : !t -> {elem}
        %w = neptune_ir.access %p0[0, -1] : !t -> {elem}
        %e = neptune_ir.access %p0[0, 1] : !t -> {elem}
        %q = arith.constant {q} : {elem}
        %a0 = arith.addf %n, %s : {elem}
        %a1 = arith.addf %a0, %w : {elem}
        %a2 = arith.addf %a1, %e : {elem}
        %av = arith.mulf %a2, %q : {elem}
        %d = arith.subf %av, %c : {elem}
        %y = math.absf %d : {elem}
"""


def np_residual(u):
    """the apply of _residual_body over the interior of u, copy-through (input 0) on the rim"""
    dt = u.dtype.type
    out = u.copy()
    a = u[:-2, 1:-1] + u[2:, 1:-1]
    a = a + u[1:-1, :-2]
    a = a + u[1:-1, 2:]
    out[1:-1, 1:-1] = np.abs(a * dt(0.25) - u[1:-1, 1:-1])
    return out


def _pointwise_body(elem, rank, tail):
    """d = p0 - p1 at the centre, then `tail`: absf -> |d|, sq -> d*d, id -> d"""
    z = ", ".join("0" * rank)
    last = {"absf": f"        %y = math.absf %d : {elem}\n", "sq": f"        %y = arith.mulf %d, %d : {elem}\n", "id": ""}[tail]
    return (f"        %x0 = neptune_ir.access %p0[{z}] : !t -> {elem}\n        %x1 = neptune_ir.access %p1[{z}] : !t -> {elem}\n"
            f"        %{'d' if tail != 'id' else 'y'} = arith.subf %x0, %x1 : {elem}\n" + last)


def fused_kinds_module(elem, box, bounds, reduce_box, body, nin, kinds, option=True):
    """@<kind>(ins...) -> elem: reduce {kind}(apply(ins){body}) over reduce_box (None: the whole result), the apply
    result used once, so the lowering fuses the two into one kernel.  All inputs share `box`."""
    rank = len(box[0])
    mr = _mr(rank, elem)
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    bargs = ", ".join(f"%p{k}: !t" for k in range(nin))
    params = ", ".join(f"%a{k}: {mr}" for k in range(nin))
    loads = "".join(f"    %g{k} = neptune_ir.wrap %a{k} : {mr} -> !f\n    %u{k} = neptune_ir.load %g{k} : !f -> !t\n" for k in range(nin))
    where = "" if reduce_box is None else f" in {_bnd(reduce_box)}"
    funcs = []
    for kind in kinds:
        funcs.append(f"""  func.func @{kind}({params}) -> {elem} {{
{loads}    %r = neptune_ir.apply({', '.join(f'%u{k}' for k in range(nin))}) attributes {{bounds = {_bnd(bounds)}}} : ({', '.join(['!t'] * nin)}) -> !t {{
      ^bb0({idx}, {bargs}):
{body}        neptune_ir.yield %y : {elem}
    }}
    %s = neptune_ir.reduce %r{where} {{kind = "{kind}"}} : !t -> {elem}
    func.return %s : {elem}
  }}
""")
    return f"""{OPTION if option else ""}#l = #neptune_ir.location<"cell">
!t = !neptune_ir.temp<element = {elem}, bounds = {_bnd(box)}, location = #l>
!f = !neptune_ir.field<element = {elem}, bounds = {_bnd(box)}, location = #l>
module {{
{"".join(funcs)}}}
"""


def residual_module(elem, shape=(34, 70)):
    """max / min / l1 / l2 of |A(u) - u|: apply.bounds the interior, the reduce over the whole box (the rim is
    copy-through: input 0 itself).  A 5-point body: the non-vector kernel."""
    box = ((0, 0), tuple(shape))
    interior = ((1, 1), (shape[0] - 1, shape[1] - 1))
    return fused_kinds_module(elem, box, interior, None, _residual_body(elem), 1, KINDS)


def pointwise_module(elem, shape, tail, kinds, reduce_box=None, bounds=None):
    """kinds of the two-input pointwise body (see _pointwise_body) over the whole box: the vector kernel when rows are
    whole 16-byte vectors"""
    box = ((0,) * len(shape), tuple(shape))
    return fused_kinds_module(elem, box, bounds or box, reduce_box, _pointwise_body(elem, len(shape), tail), 2, kinds)
