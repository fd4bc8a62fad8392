"""Module texts for the group tests (sibling applies over shared inputs run as one multi-output launch): the two committed
system fixtures resized, retyped and varied, and the slab trick that lets the oracle check planes of a production-size run."""
import re
from pathlib import Path

import numpy as np

SYSTEMS = Path(__file__).resolve().parent / "mlir_tests" / "systems"
FIXTURES = {"swe": "swe-2d-3out.mlir", "pair": "pair-3d-2out.mlir"}
NOUT = {"swe": 3, "pair": 2}


def fixture_text(kind):
    return (SYSTEMS / FIXTURES[kind]).read_text()


def variant(kind, shape, lb=None, ub=None, elem="f64"):
    """the fixture on a box of `shape` with apply.bounds [lb, ub) (default: the interior) and element type `elem`"""
    text = fixture_text(kind)
    lb = [1] * len(shape) if lb is None else list(lb)
    ub = [n - 1 for n in shape] if ub is None else list(ub)
    zeros = ", ".join("0" for _ in shape)
    text, n1 = re.subn(r"#b   = #neptune_ir.bounds<[^>]*>", f"#b   = #neptune_ir.bounds<lb = [{zeros}], ub = [{', '.join(map(str, shape))}]>", text)
    text, n2 = re.subn(r"#bi  = #neptune_ir.bounds<[^>]*>",
                       f"#bi  = #neptune_ir.bounds<lb = [{', '.join(map(str, lb))}], ub = [{', '.join(map(str, ub))}]>", text)
    assert n1 == 1 and n2 == 1
    return text.replace("f64", elem)


def inputs(kind, shape, dtype, seed=11):
    """deterministic inputs; the shallow-water depth h is kept in [1.25, 1.75) so that no division makes a NaN (whose
    sign differs between processors)"""
    import helpers
    n = NOUT[kind]
    ins = [helpers.hash_field(shape, dtype, seed=seed + k) for k in range(n)]
    if kind == "swe":
        ins[0] = (ins[0] * dtype(0.25) + dtype(1.5)).astype(dtype)
    return ins


def oracle_run(text, shape, dtype, ins, fill=-7.0):
    from helpers import oracle
    outs = [np.full(shape, fill, dtype=dtype) for _ in ins]
    oracle.Module.parse(text).call("entry", *outs, *ins)
    return outs


def oracle_band(kind, shape, lb, ub, dtype, ins, g0, g1):
    """results of rows / planes [g0, g1) along dim 0 of the full problem, computed by the oracle on the slab that holds them
    and one halo layer each side (the fixtures reach +-1 and use no index argument, so a slab is a problem of its own)"""
    n = shape[0]
    s0, s1 = max(g0 - 1, 0), min(g1 + 1, n)
    sub = (s1 - s0,) + tuple(shape[1:])
    l0 = max(lb[0], s0 + (1 if s0 > 0 else 0)) - s0
    u0 = min(ub[0], s1 - (1 if s1 < n else 0)) - s0
    if u0 < l0:
        u0 = l0
    text = variant(kind, sub, [l0] + list(lb[1:]), [u0] + list(ub[1:]), "f64" if dtype == np.float64 else "f32")
    outs = oracle_run(text, sub, dtype, [np.ascontiguousarray(a[s0:s1]) for a in ins])
    return [o[g0 - s0:g1 - s0] for o in outs]
