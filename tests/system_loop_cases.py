"""Cases for the system step loop (neptune_hip_step_loop_system on a group's geometry-level entry): inputs that stay finite
over many steps, the oracle iterated step by step, and a shallow-water variant with a fixed fourth input."""
import numpy as np

import group_cases as gc
import helpers

# member m's inputs as indices into the group's union inputs (each member lists its own unknown first; the fixtures'
# apply operands)
MEMBER_INPUTS = {"swe": [[0, 1, 2], [1, 0, 2], [2, 0, 1]], "pair": [[0, 1], [1, 0]]}
THROUGH = {"swe": [0, 1, 2], "pair": [0, 1]}
# small sizes of the loop tests: the oracle runs every step there
LOOP_SMALL = {"swe": (40, 128), "pair": (9, 12, 32)}
ELEMS = {"f64": np.float64, "f32": np.float32}


def loop_inputs(kind, shape, dtype):
    """Initial state of a multi-step run.  Shallow water: h = 1 + 0.1 gaussian, qx = qy = 0 -- h stays near 1 and every
    field finite over 100 steps (group_cases.inputs' hash fields do not: h crosses zero at step 5, and the sign of the NaNs
    that follow differs between processors).  The 3-D pair: the hash fields, bounded by 1.22 over 60 steps."""
    if kind != "swe":
        return gc.inputs(kind, shape, dtype)
    x = [np.arange(n, dtype=np.float64) - n / 2 for n in shape]
    r2 = (x[0][:, None] / (shape[0] / 8)) ** 2 + (x[1][None, :] / (shape[1] / 8)) ** 2
    h = (1.0 + 0.1 * np.exp(-r2)).astype(dtype)
    return [h, np.zeros(shape, dtype), np.zeros(shape, dtype)]


def fixed_field(shape, dtype):
    """the fixed fourth input of fixed_input_variant: small, so that 50 steps of nu * b move h by less than 0.02"""
    return (helpers.hash_field(shape, dtype, seed=29) * dtype(0.0078125)).astype(dtype)


def fixed_input_variant(shape, elem="f64"):
    """the shallow-water fixture whose h member also reads a fourth field %b at the centre (h' gains + nu b): four union
    inputs (%h, %qx, %qy, %b), three results -- %b is nobody's unknown.  @entry(oh, oqx, oqy, ih, iqx, iqy, ib)"""
    text = gc.variant("swe", shape)
    for old, new in (
            ("%iqy: memref<?x?xf64>) ->", "%iqy: memref<?x?xf64>, %ib: memref<?x?xf64>) ->"),
            ("    %h    = neptune_ir.load %fh  : !field -> !temp\n",
             "    %fb   = neptune_ir.wrap %ib  : memref<?x?xf64> -> !field\n"
             "    %b    = neptune_ir.load %fb  : !field -> !temp\n"
             "    %h    = neptune_ir.load %fh  : !field -> !temp\n"),
            ("%rh = neptune_ir.apply(%h, %qx, %qy) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {\n"
             "      ^bb0(%i: index, %j: index, %ah: !temp, %ax: !temp, %ay: !temp):\n",
             "%rh = neptune_ir.apply(%h, %qx, %qy, %b) attributes {bounds = #bi} : (!temp, !temp, !temp, !temp) -> !temp {\n"
             "      ^bb0(%i: index, %j: index, %ah: !temp, %ax: !temp, %ay: !temp, %ab: !temp):\n"
             "        %bc = neptune_ir.access %ab[0, 0] : !temp -> f64\n"),
            ("        %r    = arith.addf %t0, %dif : f64\n",
             "        %r0   = arith.addf %t0, %dif : f64\n"
             "        %bs   = arith.mulf %nu, %bc : f64\n"
             "        %r    = arith.addf %r0, %bs : f64\n")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    return text.replace("f64", elem)


def oracle_states(text, ins, steps, fixed=()):
    """[state 0, state 1, ..., state `steps`] of the system `text` steps (each a list of arrays in member order), by the
    oracle: one @entry call per step on swapped buffers, as a host loop would"""
    mod = helpers.oracle.Module.parse(text)
    cur = [a.copy() for a in ins]
    states = [[a.copy() for a in cur]]
    for _ in range(steps):
        nxt = [np.empty_like(a) for a in cur]
        mod.call("entry", *nxt, *cur, *fixed)
        cur = nxt
        states.append([a.copy() for a in cur])
    return states
