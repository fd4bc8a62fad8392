"""The cases whose device scalars are pinned bit for bit (tests/golden/solver_traces.json).

The replay tests of the three solvers pin the VECTORS bit for bit, but the traced scalars only to within the bound any two
summation orders may differ by.  This module lists solves whose scalars -- rr_0, every trace row, and rz_0 with a
preconditioner -- are recorded as exact bits by tools/record_solver_traces.py and compared by tests/test_solver_traces_gpu.py:
a change of the summation tree (another owner of the tail, another order of the partials) shows here and nowhere else.

No tuner or wisdom decision enters a sum: on the dot-monitored path kernel, tile and chunk are given (the march kernel on tile 0
in chunks of 3 planes where the fields are 16-byte aligned, which it requires; the direct kernel where they are not), and the
solver's own kernels have one grid per (cells, alignment).  The direct kernel is asked for with variant -1 and chunk 0, its
default form: an explicit kernel is no free choice, so neither the tuner nor stored launch choices are consulted, but that
default form is thereby PART of what the fixture pins -- a change of it moves the recorded pq / ts bits of the offset
cases, and is to be told from a change of the summation tree by the aligned cases staying put."""
import itertools

import numpy as np

import bicg_cases as bc
import cg_cases as cc
import helpers
import pcg_cases as pc

SOLVERS = ("cg", "pcg", "bicgstab")
# name: (shape, dtype, non-zero rim values in x)
PROBLEMS = {
    "f64_12x20x136": ((12, 20, 136), np.float64, False),
    "f32_12x20x136": ((12, 20, 136), np.float32, False),
    "f64_9x11x131_rim": ((9, 11, 131), np.float64, True),     # n = 12969: the 16-byte kernels' tail runs
    "f32_9x11x131": ((9, 11, 131), np.float32, False),        # n % 4 == 1: the f32 tail
}
PATHS = ("fused", "fallback")
OFFSETS = (0, 1)          # elements between the start of an allocation and the field in it
CHECK_EVERY = 3
ITERS = {np.float64: 8, np.float32: 6}
# one block long enough to be replayed from a captured graph (BiCGStab: two graphs of 4; CG, PCG: one of 8)
GRAPH_PROBLEM, GRAPH_ITERS = "f64_12x20x136", 10


def cases():
    """-> [(key, solver, problem, path, offset, iters, check_every)]"""
    out = []
    for solver, problem, path, offset in itertools.product(SOLVERS, PROBLEMS, PATHS, OFFSETS):
        key = f"{solver}/{problem}/{path}/{'aligned' if offset == 0 else 'offset%d' % offset}"
        out.append((key, solver, problem, path, offset, ITERS[PROBLEMS[problem][1]], CHECK_EVERY))
    for solver in SOLVERS:
        out.append((f"{solver}/{GRAPH_PROBLEM}/fused/aligned/graph", solver, GRAPH_PROBLEM, "fused", 0, GRAPH_ITERS, GRAPH_ITERS))
    return out


def offset_field(nh, a, elems):
    """a field holding `a` that starts `elems` elements into a larger allocation"""
    dtype = nh.fields._FROM_NP[a.dtype]
    big = nh.torch.empty(a.size + elems, dtype=nh.fields._TORCH_DTYPE[dtype], device="cuda")
    view = big[elems:].view(a.shape)
    view.copy_(nh.torch.from_numpy(np.ascontiguousarray(a)))
    f = nh.fields.DeviceField((0,) * a.ndim, a.shape, dtype, view)
    assert f.ptr == big.data_ptr() + elems * a.itemsize
    return f


class _Problem:
    pass


def _problem(nh, cache, solver, name):
    """the compiled operator and the host arrays of one (solver, problem): built once, left unchanged"""
    if (solver, name) not in cache:
        shape, dtype, rim = PROBLEMS[name]
        if solver == "pcg":
            P = pc.Problem(shape, dtype, rim=rim)
        elif solver == "bicgstab":
            P = bc.Problem(shape, dtype, rim=rim)
        else:
            P = _Problem()
            P.shape, P.dtype, P.text, P.bounds = shape, dtype, cc.cg_module(shape, dtype), cc.interior(shape)
            P.b = helpers.hash_field(shape, dtype, seed=71)
            P.x0 = helpers.hash_field(shape, dtype, seed=72) if rim else np.zeros(shape, dtype)
        P.entry = nh.lowering.compile_module(P.text, dot_entries=True).dot_entry("entry")
        cache[(solver, name)] = P
    return cache[(solver, name)]


def run(nh, cache, case):
    """one solve on the device -> {"rr0": hex, "trace": [[hex, ...], ...]} and, with a preconditioner, "rz0": hex.  nh: a
    namespace with torch, capi, apply, fields and lowering; cache: a dict that keeps the compiled operators."""
    key, solver, name, path, offset, iters, check_every = case
    P = _problem(nh, cache, solver, name)
    F, K = nh.fields.DeviceField, nh.capi
    make = (lambda a: offset_field(nh, a, offset)) if offset else F.from_numpy
    nan = np.full(P.shape, np.nan, P.dtype)
    x, b = make(P.x0), make(P.b)
    work = [make(nan) for _ in range(5 if solver == "bicgstab" else 3)]
    cfg = None
    if path == "fused":
        cfg = nh.apply.make_cfg(K.KERNEL_MARCH, 0, 3) if offset == 0 else nh.apply.make_cfg(K.KERNEL_DIRECT, -1, 0)
    kw = dict(check_every=check_every, trace=True, dot="auto" if path == "fused" else "fallback", cfg=cfg, work=work)
    if solver == "bicgstab":
        done, rr0, rr_last, trace = nh.apply.bicgstab_solve(P.entry, x, b, P.bounds, iters, 0.0, **kw)
    elif solver == "pcg":
        done, rr0, rr_last, trace = nh.apply.cg_solve(P.entry, x, b, P.bounds, iters, 0.0, others=[F.from_numpy(P.w)],
                                                      minv=make(P.minv), **kw)
    else:
        done, rr0, rr_last, trace = nh.apply.cg_solve(P.entry, x, b, P.bounds, iters, 0.0, **kw)
    nh.torch.cuda.synchronize()
    counts = nh.apply.cg_counts()
    assert done == iters and counts[:2] == ((iters, 0) if path == "fused" else (0, iters)), (key, done, counts)
    out = {"rr0": float(rr0).hex(), "trace": [[float(v).hex() for v in row] for row in trace]}
    if solver == "pcg":
        out["rz0"] = float(nh.apply.pcg_rz0()).hex()
    return out
