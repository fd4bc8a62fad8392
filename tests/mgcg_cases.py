"""The problems of multigrid-preconditioned conjugate gradients (neptune_hip_mgcg_solve): the anisotropic star
and hierarchies whose level 0 has minv = +0 outside Omega -- the preconditioner's first pre-sweep is z = minv_0 * r on EVERY
cell of the box.  The preconditioner, the set-up and the replay are mg_restatement's."""
import numpy as np

import mg_cases as mgc
import mg_restatement as rst
import monitor_cases as mc


# ---------------------------------------------------------------- the anisotropic star
def aniso_module(shape, weights, dtype=np.float64, bounds=None):
    """NeptuneIR text of @entry(out, in): out<p> = (2 * sum of weights) * u<p> - sum over axes d of weights[d] * (u<p - e_d> +
    u<p + e_d>) one cell in from every face, copy-through on the rim: the unscaled operator -sum_d weights[d] u_dd, with
    its own side weight per axis (mg_cases.mg_module is weights = 1 everywhere, in another order of additions).
    bounds: (lb, ub) of the apply instead of one cell in from every face"""
    rank = len(shape)
    assert len(weights) == rank
    if bounds is None:
        bounds = ([1] * rank, [n - 1 for n in shape])
    elem = mc.ELEM[np.dtype(dtype)]
    lst = lambda v: ", ".join(str(int(x)) for x in v)
    mr = "x".join(["?"] * rank) + "x" + elem
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    zero = [0] * rank
    body = [f"        %c = neptune_ir.access %a[{lst(zero)}] : !temp -> {elem}",
            f"        %wc = arith.constant {float(2.0 * sum(float(w) for w in weights))!r} : {elem}",
            f"        %acc0 = arith.mulf %wc, %c : {elem}"]
    for d in range(rank):
        lo, hi = list(zero), list(zero)
        lo[d], hi[d] = -1, 1
        body += [f"        %m{d} = neptune_ir.access %a[{lst(lo)}] : !temp -> {elem}",
                 f"        %p{d} = neptune_ir.access %a[{lst(hi)}] : !temp -> {elem}",
                 f"        %s{d} = arith.addf %m{d}, %p{d} : {elem}",
                 f"        %w{d} = arith.constant {-float(weights[d])!r} : {elem}",
                 f"        %t{d} = arith.mulf %w{d}, %s{d} : {elem}",
                 f"        %acc{d + 1} = arith.addf %acc{d}, %t{d} : {elem}"]
    body.append(f"        neptune_ir.yield %acc{rank} : {elem}")
    out = ['#loc = #neptune_ir.location<"cell">',
           f"#b   = #neptune_ir.bounds<lb = [{lst(zero)}], ub = [{lst(shape)}]>",
           f"#bi  = #neptune_ir.bounds<lb = [{lst(bounds[0])}], ub = [{lst(bounds[1])}]>",
           f"!temp  = !neptune_ir.temp<element = {elem}, bounds = #b, location = #loc>",
           f"!field = !neptune_ir.field<element = {elem}, bounds = #b, location = #loc>",
           "module {",
           f"  func.func @entry(%out: memref<{mr}>, %in: memref<{mr}>) -> memref<{mr}> {{",
           f"    %fout = neptune_ir.wrap %out : memref<{mr}> -> !field",
           f"    %fu   = neptune_ir.wrap %in : memref<{mr}> -> !field",
           "    %u    = neptune_ir.load %fu : !field -> !temp",
           "    %r = neptune_ir.apply(%u) attributes {bounds = #bi} : (!temp) -> !temp {",
           f"      ^bb0({idx}, %a: !temp):"] + body + ["      }",
           "    neptune_ir.store %r to %fout : !temp to !field",
           f"    %res  = neptune_ir.unwrap %fout : !field -> memref<{mr}>",
           f"    func.return %res : memref<{mr}>",
           "  }", "}"]
    return "\n".join(out) + "\n"


def aniso_levels(omega, n_levels, weights, damp, dtype=np.float64, minv_outside=0.0):
    """restatement levels of the anisotropic star on whole-interior boxes (rim of one cell), damped-Jacobi weights
    damp / diagonal on Omega and `minv_outside` elsewhere; -> (levels, module texts)"""
    dt = np.dtype(dtype).type
    shapes = mgc.level_shapes(omega, n_levels)
    texts = [aniso_module(shape, weights, dtype) for shape, _ in shapes]
    levels = []
    for text, (shape, where) in zip(texts, shapes):
        minv = np.full(shape, minv_outside, dtype)
        minv[where] = dt(dt(damp) / dt(2.0 * sum(float(w) for w in weights)))
        levels.append(rst.Level(rst.Operator(text), shape, where, minv, dtype))
    return levels, texts


def star_levels(omega, n_levels, dtype, damp, texts=None):
    """mg_cases.star_levels with the weights this solver needs: level 0's minv is +0 outside Omega (the definition forms
    z = minv_0 * r on the whole box), the coarser levels' stay NaN there (never read); -> (levels, module texts)"""
    levels, texts = mgc.star_levels(omega, n_levels, dtype, damp, texts=texts)
    L0 = levels[0]
    L0.minv = mgc.minv_field(L0.shape, L0.where, dtype, damp, outside=0.0)
    return levels, texts
