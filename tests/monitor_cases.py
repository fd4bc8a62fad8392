"""Modules and reference sums of the monitored-apply tests: weighted star stencils of rank 1..3 as NeptuneIR
text -- @entry(out, in) applies the operator once --, the update norm S = sum (new - old)^2 as the issue defines it, computed
from the oracle's fields in numpy, and the bound two summation orders of the same terms may differ by."""
import math

import numpy as np

ELEM = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}


def star_module(shape, dtype=np.float64, origin=None, bounds=None, radius=1, centre=0.5, side=None, second_input=False,
                shifted_input0=False, halo_on_second=False):
    """out<p> = centre * u<p> + side * (sum of the 2 * rank * radius star neighbours of u at p) [+ 0.25 * v<p>] over `bounds`
    (default: `radius` cells in from every face), copy-through elsewhere.  Weights are powers of two or small dyadic
    numbers, so every product is exact in f32 and f64 alike.  side defaults to 1 / (8 * rank * radius): with centre = 0.5 the
    absolute weights sum to 0.75 < 1 -- a contraction, S falls steadily under iteration.
    halo_on_second: the neighbours are read from a second input v instead (no 0.25 * v term): input 0 is read at the centre
    only, so what it holds outside `bounds` never reaches a cell inside.
    shifted_input0: input 0 lives in a box of the same shape one cell further along dim 0 than the result's."""
    rank = len(shape)
    elem = ELEM[np.dtype(dtype)]
    origin = [0] * rank if origin is None else [int(x) for x in origin]
    if bounds is None:
        bounds = ([o + radius for o in origin], [o + n - radius for o, n in zip(origin, shape)])
    if side is None:
        side = 1.0 / (8 * rank * radius)
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    ub = [o + n for o, n in zip(origin, shape)]
    in_lb = [origin[0] + 1] + origin[1:] if shifted_input0 else origin
    in_ub = [ub[0] + 1] + ub[1:] if shifted_input0 else ub
    mr = "x".join(["?"] * rank) + "x" + elem
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    acc, names = [f"        %c = neptune_ir.access %a[{lst([0] * rank)}] : !tin -> {elem}"], []
    for d in range(rank):
        for r in range(1, radius + 1):
            for sgn, tag in ((-1, "m"), (1, "p")):
                off = [0] * rank
                off[d] = sgn * r
                nm = f"n{d}{tag}{r}"
                names.append(nm)
                acc.append(f"        %{nm} = neptune_ir.access %o[{lst(off)}] : !temp -> {elem}" if halo_on_second else
                           f"        %{nm} = neptune_ir.access %a[{lst(off)}] : !tin -> {elem}")
    ops = [f"        %wc = arith.constant {float(centre)!r} : {elem}", f"        %ws = arith.constant {float(side)!r} : {elem}"]
    prev = names[0]
    for t, nm in enumerate(names[1:]):
        ops.append(f"        %s{t} = arith.addf %{prev}, %{nm} : {elem}")
        prev = f"s{t}"
    ops += [f"        %t0 = arith.mulf %wc, %c : {elem}", f"        %t1 = arith.mulf %ws, %{prev} : {elem}",
            f"        %t2 = arith.addf %t0, %t1 : {elem}"]
    res = "t2"
    if halo_on_second:
        second_input = True
    elif second_input:
        acc.append(f"        %vc = neptune_ir.access %o[{lst([0] * rank)}] : !temp -> {elem}")
        ops += [f"        %wv = arith.constant 0.25 : {elem}", f"        %t3 = arith.mulf %wv, %vc : {elem}",
                f"        %t4 = arith.addf %t2, %t3 : {elem}"]
        res = "t4"
    ops.append(f"        neptune_ir.yield %{res} : {elem}")
    ins = "%u, %v" if second_input else "%u"
    in_types = "(!tin, !temp)" if second_input else "(!tin)"
    region_args = f"{idx}, %a: !tin" + (", %o: !temp" if second_input else "")
    extra_arg = f", %in1: memref<{mr}>" if second_input else ""
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(origin)}], ub = [{lst(ub)}]>",
           f"#bin = #neptune_ir.bounds<lb = [{lst(in_lb)}], ub = [{lst(in_ub)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst(bounds[0])}], ub = [{lst(bounds[1])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           f"!tin   = !neptune_ir.temp<element = {elem}, bounds = #bin, location = #loc>",
           f"!fin   = !neptune_ir.field<element = {elem}, bounds = #bin, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>{extra_arg}) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !fin",
           "    %u    = neptune_ir.load %fu : !fin -> !tin"]
    if second_input:
        out += [f"    %fv   = neptune_ir.wrap %in1 : memref<{mr}> -> !field", "    %v    = neptune_ir.load %fv : !field -> !temp"]
    out += [f"    %r = neptune_ir.apply({ins}) attributes {{bounds = #bi}} : {in_types} -> !temp {{",
            f"      ^bb0({region_args}):"] + acc + ops + ["      }",
            "    neptune_ir.store %r to %fout : !temp to !field",
            f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
            f"    func.return %res : memref<{mr}>",
            "  }", "}"]
    return "\n".join(out) + "\n"


def inside_slices(shape, origin, bounds, region0=None):
    """numpy index of apply.bounds (logical) x launch region (a dim-0 range, physical) in a field of `shape` at `origin`"""
    sl = []
    for d, (o, n) in enumerate(zip(origin, shape)):
        lo, hi = max(bounds[0][d] - o, 0), min(bounds[1][d] - o, n)
        if d == 0 and region0 is not None:
            lo, hi = max(lo, region0[0]), min(hi, region0[1])
        sl.append(slice(lo, max(hi, lo)))
    return tuple(sl)


def reference_sum(new: np.ndarray, old: np.ndarray, where):
    """-> (S, bound): the terms (new - old), then squared, each rounded once in the fields' element type, summed exactly
    (math.fsum); bound = 2 (n - 1) eps sum |x_i|, what any two summation orders of these n terms may differ by
    (tests/test_reduce_gpu.py)"""
    dt = new.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        d = (new[where] - old[where]).astype(dt)
        terms = (d * d).astype(dt)
    flat = [float(x) for x in terms.ravel()]
    n = len(flat)
    s = math.fsum(flat) if n else 0.0
    bound = 2.0 * max(n - 1, 0) * float(np.finfo(dt).eps) * math.fsum(abs(x) for x in flat) if n else 0.0
    return s, bound
