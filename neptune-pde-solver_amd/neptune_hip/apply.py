"""Host-side launch of the apply hot path through the C ABI (neptune_hip_apply_builtin & co).

This is the thin layer the Python frontend, the tests and the bench share; it mirrors what the
emitted host C++ of a lowered module does for one `neptune_ir.apply` + `neptune_ir.store`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from . import _capi
from .fields import DeviceField, current_stream_ptr
from .geometry import Box, make_geom

BODY_BY_NAME = {
    "lap2d5_f64": _capi.BODY_LAP2D5_F64,
    "lap3d7_f64": _capi.BODY_LAP3D7_F64,
    "lap3d27_f32": _capi.BODY_LAP3D27_F32,
    "lap1d3_f64": _capi.BODY_LAP1D3_F64,
}
BODY_DTYPE = {_capi.BODY_LAP2D5_F64: _capi.F64, _capi.BODY_LAP3D7_F64: _capi.F64,
              _capi.BODY_LAP3D27_F32: _capi.F32, _capi.BODY_LAP1D3_F64: _capi.F64}
BODY_RANK = {_capi.BODY_LAP2D5_F64: 2, _capi.BODY_LAP3D7_F64: 3, _capi.BODY_LAP3D27_F32: 3,
             _capi.BODY_LAP1D3_F64: 1}
BODY_POINTS = {_capi.BODY_LAP2D5_F64: 5, _capi.BODY_LAP3D7_F64: 7, _capi.BODY_LAP3D27_F32: 27,
               _capi.BODY_LAP1D3_F64: 3}


def _in_array(inputs: Sequence[DeviceField]):
    arr = (C.c_void_p * len(inputs))(*[f.ptr for f in inputs])
    return arr


def make_cfg(kernel: int = _capi.KERNEL_AUTO, variant: int = -1, chunk: int = 0, flags: int = 0) -> _capi.LaunchCfg:
    """variant -1 = the library's default tile for the stencil shape; flags: _capi.FLAG_DIRECT_FLAT"""
    return _capi.LaunchCfg(kernel, variant, chunk, flags)


def geom_for(inputs: Sequence[DeviceField], out: DeviceField, bounds: Box, region: Optional[Box] = None):
    return make_geom(out.box, bounds, [f.box for f in inputs], region)


def apply_builtin(body, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box,
                  region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None,
                  stream: Optional[int] = None) -> None:
    """out = apply(inputs) {bounds}; asynchronous on `stream`.  `body`: a built-in body id, or the geometry-level
    entry of a lowered module's apply (neptune_hip.lowering.LoweredModule.geom_entry)."""
    lib = _capi.load()
    g = geom_for(inputs, out, bounds, region)
    st = current_stream_ptr() if stream is None else stream
    if hasattr(body, "fn"):
        rc = body(g, _in_array(inputs), out.ptr, st, cfg)
        _capi.check(rc, body.symbol)
        return
    rc = lib.neptune_hip_apply_builtin(body, C.byref(g), _in_array(inputs), out.ptr, st,
                                       C.byref(cfg) if cfg is not None else None)
    _capi.check(rc, "neptune_hip_apply_builtin")


def step_loop(body, a: DeviceField, b: DeviceField, bounds: Box, steps: int, others: Sequence[DeviceField] = (),
              cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None) -> DeviceField:
    """`steps` applies in a row, ping-ponging between fields a and b (step 0 reads a); `others` are the fixed
    inputs 1.. of a multi-input body.  The pair of launches is captured once into a hipGraph and replayed, so small
    fields are not bound by launch overhead.  Asynchronous; returns the field holding the newest state."""
    lib = _capi.load()
    g = geom_for([a] + list(others), b, bounds)
    fields2 = (C.c_void_p * 2)(a.ptr, b.ptr)
    ins = _in_array([a] + list(others))
    st = current_stream_ptr() if stream is None else stream
    is_entry = hasattr(body, "fn")
    fn = C.cast(body.fn, C.c_void_p) if is_entry else None
    fn2 = C.cast(body.fn2, C.c_void_p) if is_entry and getattr(body, "fn2", None) is not None else None
    fn3 = C.cast(body.fn3, C.c_void_p) if is_entry and getattr(body, "fn3", None) is not None else None
    rc = lib.neptune_hip_step_loop_chain(fn, fn2, fn3, -1 if is_entry else body, C.byref(g), fields2, ins, steps, st,
                                         C.byref(cfg) if cfg is not None else None)
    _capi.check(rc, "neptune_hip_step_loop_chain")
    return b if steps % 2 else a


def apply_norm(body, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box, sum_out=None,
               region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None):
    """a monitored launch: out = apply(inputs) {bounds} exactly as apply_builtin computes it, and S = sum (new - old)^2 over
    the cells of `bounds` in the launch region (old = inputs[0] at the same physical index) in the field's element type.
    `body`: a built-in body id, or the norm entry of a lowered apply (LoweredModule.norm_entry).  `sum_out`: a one-element
    torch CUDA tensor of the field's element type that receives S in stream order (asynchronous; returns it), or None:
    one is allocated, the call synchronises and returns S as a float.  Returns None -- having launched nothing -- when
    the request has no monitored form (a plan onto the plane-in-LDS kernels: NEPTUNE_HIP_EUNSUPPORTED)."""
    import torch
    lib = _capi.load()
    g = geom_for(inputs, out, bounds, region)
    st = current_stream_ptr() if stream is None else stream
    dst = sum_out if sum_out is not None else torch.empty(1, dtype=out.tensor.dtype, device=out.tensor.device)
    cfg_p = C.byref(cfg) if cfg is not None else None
    if hasattr(body, "fn"):
        if body.fn_norm is None:
            raise ValueError(f"{body.symbol}: no monitored launch (compile the module with norm_entries=True)")
        rc, what = body.fn_norm(C.byref(g), _in_array(inputs), out.ptr, dst.data_ptr(), st, cfg_p), body.symbol
    else:
        rc = lib.neptune_hip_apply_builtin_norm(body, C.byref(g), _in_array(inputs), out.ptr, dst.data_ptr(), st, cfg_p)
        what = "neptune_hip_apply_builtin_norm"
    if rc == _capi.EUNSUPPORTED:
        return None
    _capi.check(rc, what)
    if sum_out is not None:
        return sum_out
    torch.cuda.synchronize()
    return float(dst.item())


def until_loop_counts():
    """(checked steps run as monitored launches, checked steps run as plain launch + two-field reduction, checks) of the
    last step_loop_until call"""
    fused, fallback, checks = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_until_loop_counts(C.byref(fused), C.byref(fallback), C.byref(checks))
    return fused.value, fallback.value, checks.value


def step_loop_until(body, a: DeviceField, b: DeviceField, bounds: Box, max_steps: int, tol2: float, check_every: int = 1,
                    others: Sequence[DeviceField] = (), norm="auto", cfg: Optional[_capi.LaunchCfg] = None,
                    stream: Optional[int] = None):
    """iterate u <- A(u), ping-ponging between fields a and b (step 0 reads a), until S = sum (A(u) - u)^2 <= tol2 -- the
    threshold is on S itself, no square root -- or max_steps steps have run.  S is taken every `check_every` steps, out of
    the checked step's own launch where a monitored form exists.  `body`: a built-in body id or a lowered apply's
    geometry-level entry (LoweredModule.geom_entry); `norm`: that apply's norm entry (LoweredModule.norm_entry), None for
    the fallback (plain launch + one read-only pass over both fields), "auto": body's own (built-in bodies have one).
    Blocking; -> (steps_done, last_sum).  The newest state is in (a, b)[steps_done % 2]; the other field holds state
    steps_done - 1.  A NaN sum never satisfies the test.  until_loop_counts() tells which path the checks took."""
    lib = _capi.load()
    g = geom_for([a] + list(others), b, bounds)
    fields2 = (C.c_void_p * 2)(a.ptr, b.ptr)
    ins = _in_array([a] + list(others))
    st = current_stream_ptr() if stream is None else stream
    is_entry = hasattr(body, "fn")
    fn = C.cast(body.fn, C.c_void_p) if is_entry else None
    if isinstance(norm, str):   # "auto"
        norm = body if is_entry else None
    fn_norm = C.cast(norm.fn_norm, C.c_void_p) if (is_entry and norm is not None and norm.fn_norm is not None) else None
    done, last = C.c_int64(0), C.c_double(0.0)
    rc = lib.neptune_hip_step_loop_until(fn, fn_norm, -1 if is_entry else body, a.dtype, C.byref(g), fields2, ins, max_steps,
                                         check_every, tol2, st, C.byref(cfg) if cfg is not None else None, C.byref(done),
                                         C.byref(last))
    _capi.check(rc, "neptune_hip_step_loop_until")
    return done.value, last.value


def apply_dot(body, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box, dot_out=None,
              region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None):
    """a dot-monitored launch: out = apply(inputs) {bounds} exactly as apply_builtin computes it, and D = sum new * old over
    the cells of `bounds` in the launch region (old = inputs[0] at the same physical index, one rounding per product) in the
    field's element type -- p . A(p) when inputs[0] = p.  `body`: a built-in body id, or the dot entry of a lowered apply
    (LoweredModule.dot_entry).  `dot_out`, the return value and the refusal (None, nothing launched): as apply_norm."""
    import torch
    lib = _capi.load()
    g = geom_for(inputs, out, bounds, region)
    st = current_stream_ptr() if stream is None else stream
    dst = dot_out if dot_out is not None else torch.empty(1, dtype=out.tensor.dtype, device=out.tensor.device)
    cfg_p = C.byref(cfg) if cfg is not None else None
    if hasattr(body, "fn"):
        if body.fn_dot is None:
            raise ValueError(f"{body.symbol}: no dot-monitored launch (compile the module with dot_entries=True)")
        rc, what = body.fn_dot(C.byref(g), _in_array(inputs), out.ptr, dst.data_ptr(), st, cfg_p), body.symbol
    else:
        rc = lib.neptune_hip_apply_builtin_dot(body, C.byref(g), _in_array(inputs), out.ptr, dst.data_ptr(), st, cfg_p)
        what = "neptune_hip_apply_builtin_dot"
    if rc == _capi.EUNSUPPORTED:
        return None
    _capi.check(rc, what)
    if dot_out is not None:
        return dot_out
    torch.cuda.synchronize()
    return float(dst.item())


def dot(a: DeviceField, b: DeviceField, bounds: Box, region: Optional[Box] = None, dot_out=None, stream: Optional[int] = None):
    """sum a * b over the cells of `bounds` in the launch region, in one read-only pass (neptune_hip_dot): what apply_dot
    returns for out = a, inputs[0] = b, in another summation order.  `dot_out` and the return value: as apply_dot."""
    import torch
    lib = _capi.load()
    g = geom_for([b], a, bounds, region)
    st = current_stream_ptr() if stream is None else stream
    dst = dot_out if dot_out is not None else torch.empty(1, dtype=a.tensor.dtype, device=a.tensor.device)
    _capi.check(lib.neptune_hip_dot(a.dtype, C.byref(g), a.ptr, b.ptr, dst.data_ptr(), st), "neptune_hip_dot")
    if dot_out is not None:
        return dot_out
    torch.cuda.synchronize()
    return float(dst.item())


def cg_counts():
    """(iterations whose q = A(p) ran as a dot-monitored launch, iterations that ran plain launch + neptune_hip_dot, read-backs
    after blocks of iterations) of the last cg_solve or bicgstab_solve call (for BiCGStab the launch in question is t = A(s))"""
    fused, fallback, checks = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_cg_counts(C.byref(fused), C.byref(fallback), C.byref(checks))
    return fused.value, fallback.value, checks.value


def resolve_dot(who: str, entry, dot):
    """a solver's `dot` argument -- "auto", "fallback", None or a dot entry -- as the fn_dot pointer to hand the C entry, or
    None: a plain launch and a separate dot product.  entry: the operator (only a lowered entry can have one to hand over; a
    built-in body's is the library's own).  who: the caller's name in the error text."""
    is_entry = hasattr(entry, "fn")
    if isinstance(dot, str):
        if dot not in ("auto", "fallback"):
            raise ValueError(f'{who}: dot is "auto", "fallback", None or a dot entry')
        dot = entry if (dot == "auto" and is_entry) else None
    return C.cast(dot.fn_dot, C.c_void_p) if (is_entry and dot is not None and dot.fn_dot is not None) else None


def trace_buffer(cols: int, max_iters: int, like_tensor, dtype=None):
    """a zeroed device tensor for a solver's trace: `cols` values per iteration (never empty), on like_tensor's device and
    of its element type unless `dtype` says otherwise"""
    import torch
    return torch.zeros(cols * max(int(max_iters), 1), dtype=dtype or like_tensor.dtype, device=like_tensor.device)


def _krylov_solve(entry, x, b, bounds, max_iters, tol2, check_every, others, trace, dot, cfg, work, region, stream, *,
                  who, symbol, n_work, out_index, cols, extra=()):
    """what cg_solve and bicgstab_solve share: the entries, the geometry (the field work[out_index] receives the operator's
    result), the n_work work fields and the trace of `cols` values per iteration, then the C entry `symbol`(fn, fn_dot, body,
    dtype, g, x, b, *extra, work, ...) and the result tuple.  who: the caller's name in error texts."""
    lib = _capi.load()
    others = list(others)
    if work is None:
        work = [DeviceField.empty_like(x) for _ in range(n_work)]
    g = geom_for([x] + others, work[out_index], bounds, region)
    st = current_stream_ptr() if stream is None else stream
    is_entry = hasattr(entry, "fn")
    fn = C.cast(entry.fn, C.c_void_p) if is_entry else None
    fn_dot = resolve_dot(who, entry, dot)
    tr = trace_buffer(cols, max_iters, x.tensor) if trace else None
    warr = (C.c_void_p * n_work)(*[f.ptr for f in work])
    rest = _in_array(others) if others else None
    done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    rc = getattr(lib, symbol)(fn, fn_dot, -1 if is_entry else entry, x.dtype, C.byref(g), x.ptr, b.ptr, *extra, warr, rest,
                              max_iters, check_every, tol2, tr.data_ptr() if trace else None, st,
                              C.byref(cfg) if cfg is not None else None, C.byref(done), C.byref(rr0), C.byref(last))
    _capi.check(rc, symbol)
    if trace:
        return done.value, rr0.value, last.value, tr.cpu().numpy()[:cols * done.value].reshape(-1, cols)
    return done.value, rr0.value, last.value


def cg_solve(entry, x: DeviceField, b: DeviceField, bounds: Box, max_iters: int, tol2: float, check_every: int = 1,
             others: Sequence[DeviceField] = (), trace: bool = False, dot="auto", cfg: Optional[_capi.LaunchCfg] = None,
             work: Optional[Sequence[DeviceField]] = None, region: Optional[Box] = None, stream: Optional[int] = None,
             minv: Optional[DeviceField] = None):
    """solve A(x) = b by conjugate gradients on the device (neptune_hip_cg_solve): `entry` is a built-in body id or a lowered
    apply's geometry-level entry whose input 0 has the result's box; `others` are its fixed inputs 1...  x: initial guess in,
    solution out; its cells outside `bounds` (x region) are boundary data and are never written.  The loop stops when
    r . r <= tol2 (checked every `check_every` iterations) or after max_iters iterations.  dot: the apply's dot entry
    (LoweredModule.dot_entry), "auto": entry's own if it has one (built-in bodies do), "fallback" or None: a plain launch
    and a separate dot product per iteration.  work: three fields like x for r, p, q (allocated here when None).
    Blocking; -> (iters, rr0, rr_last), and with trace=True a fourth item: a numpy array of shape (iters, 2) holding
    (p . A(p) of iteration k, r . r after it).  cg_counts() tells which path the iterations took.
    minv: a field like x holding the inverse of a diagonal preconditioner (jacobi_minv): the solve is then
    neptune_hip_pcg_solve, tol2 still bounds the true r . r, and the trace has shape (iters, 3): (p . A(p) of iteration k,
    r . (minv r) after it, r . r after it)."""
    if minv is None:
        return _krylov_solve(entry, x, b, bounds, max_iters, tol2, check_every, others, trace, dot, cfg, work, region, stream,
                             who="cg_solve", symbol="neptune_hip_cg_solve", n_work=3, out_index=2, cols=2)
    if minv.box != x.box or minv.dtype != x.dtype:
        raise ValueError("cg_solve: minv must have the box and the element type of x")
    return _krylov_solve(entry, x, b, bounds, max_iters, tol2, check_every, others, trace, dot, cfg, work, region, stream,
                         who="cg_solve", symbol="neptune_hip_pcg_solve", n_work=3, out_index=2, cols=3, extra=(minv.ptr,))


def pcg_rz0() -> float:
    """r . (minv r) after the set-up of the last cg_solve(..., minv=...) call: with rr0 and the trace, every scalar the
    recurrences used"""
    return float(_capi.load().neptune_hip_pcg_rz0())


def bicgstab_solve(entry, x: DeviceField, b: DeviceField, bounds: Box, max_iters: int, tol2: float, check_every: int = 1,
                   others: Sequence[DeviceField] = (), trace: bool = False, dot="auto", cfg: Optional[_capi.LaunchCfg] = None,
                   work: Optional[Sequence[DeviceField]] = None, region: Optional[Box] = None, stream: Optional[int] = None):
    """solve A(x) = b by BiCGStab on the device (neptune_hip_bicgstab_solve) for an apply that need not be symmetric.  entry,
    x, b, bounds, others, max_iters, tol2 (the threshold on r . r), check_every, dot ("auto", "fallback", None or a dot entry), cfg,
    region and stream: as cg_solve.  work: five fields like x for r, rh, p, v, t (allocated here when None).
    Blocking; -> (iters, rr0, rr_last), and with trace=True a fourth item: a numpy array of shape (iters, 5) holding
    (rh . A(p), A(s) . s, A(s) . A(s) of iteration k, rh . r and r . r after it).  cg_counts() tells which path the iterations
    took."""
    if work is not None and len(work) != 5:
        raise ValueError("bicgstab_solve: work is five fields (r, rh, p, v, t)")
    return _krylov_solve(entry, x, b, bounds, max_iters, tol2, check_every, others, trace, dot, cfg, work, region, stream,
                         who="bicgstab_solve", symbol="neptune_hip_bicgstab_solve", n_work=5, out_index=3, cols=5)


def _omega(like: DeviceField, bounds: Box, region: Optional[Box]):
    """Omega = bounds (logical) x launch region (physical) as physical [lo, hi) per dimension of `like`'s box"""
    lo = [max(int(bounds[0][d]) - like.lb[d], 0 if region is None else int(region[0][d]), 0) for d in range(like.rank)]
    hi = [min(int(bounds[1][d]) - like.lb[d], like.shape[d] if region is None else int(region[1][d]), like.shape[d])
          for d in range(like.rank)]
    return lo, hi


def operator_diagonal(entry, like: DeviceField, bounds: Box, others: Sequence[DeviceField] = (), reach=None,
                      region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None) -> DeviceField:
    """the diagonal of a LINEAR operator: a field like `like` holding A's diagonal entry on the cells of
    Omega = bounds x region and +0 elsewhere.  `entry`, `others`, `bounds`, `region`: as cg_solve.  The operator is probed with
    coloured unit vectors: with s_d = 2 reach_d + 1, each of the prod s_d colours c is a field that is 1 on the cells of Omega
    whose offset from Omega's lower corner is = c (mod s) and 0 on every other cell of the box (the boundary cells too); one
    plain launch per colour, and the result is copied at exactly those cells -- two cells of one colour are further apart than
    the operator reaches, so each sees its own diagonal entry alone.  reach: an int or one int per dimension, how far A reads
    from a cell; for a lowered entry it defaults to the entry's halo0 in every dimension (right for star and box stencils of
    one radius; give it per dimension for an operator that reaches further along another dimension than along dim 0), for a
    built-in body it is required.  One more launch guards the choice: a unit vector at the middle cell of Omega must not be
    seen beyond `reach`, else ValueError (a NaN out there counts as seen).  Set-up work: prod s_d + 1 launches and torch
    indexing, blocking.
    An AFFINE operator (A(0) != 0: a source term inside the apply) gives a wrong answer: the probe returns A(0) + diagonal."""
    import itertools
    import torch
    if reach is None:
        if not hasattr(entry, "halo0"):
            raise ValueError("operator_diagonal: reach is required for a built-in body")
        reach = entry.halo0
    reach = [int(reach)] * like.rank if isinstance(reach, int) else [int(r) for r in reach]
    if len(reach) != like.rank or any(r < 0 for r in reach):
        raise ValueError("operator_diagonal: reach is a non-negative int or one per dimension")
    others = list(others)
    lo, hi = _omega(like, bounds, region)
    diag = DeviceField.empty_like(like)
    diag.tensor.zero_()
    if any(h <= l for l, h in zip(lo, hi)):
        return diag
    probe, out = DeviceField.empty_like(like), DeviceField.empty_like(like)
    stride = [2 * r + 1 for r in reach]
    # guard: one unit vector at the middle cell of Omega must come back as zeros beyond `reach` around it -- an operator that
    # reaches further there would let two cells of one colour see each other and the diagonal would be silently wrong
    mid = [(l + h) // 2 for l, h in zip(lo, hi)]
    probe.tensor.zero_()
    probe.tensor[tuple(mid)] = 1.0
    out.tensor.zero_()
    apply_builtin(entry, [probe] + others, out, bounds, region=region, cfg=cfg)
    seen = out.tensor[tuple(slice(l, h) for l, h in zip(lo, hi))].clone()
    seen[tuple(slice(max(m - r - l, 0), m + r + 1 - l) for m, r, l in zip(mid, reach, lo))] = 0.0
    if bool((seen != 0).any()):
        raise ValueError(f"operator_diagonal: the operator reaches further than reach = {reach} (a unit vector at {mid} is seen "
                         "beyond it): give reach per dimension")
    for colour in itertools.product(*[range(min(s, h - l)) for s, l, h in zip(stride, lo, hi)]):
        cells = tuple(slice(l + c, h, s) for l, h, c, s in zip(lo, hi, colour, stride))
        probe.tensor.zero_()
        probe.tensor[cells] = 1.0
        out.tensor.zero_()
        apply_builtin(entry, [probe] + others, out, bounds, region=region, cfg=cfg)
        diag.tensor[cells] = out.tensor[cells]
    torch.cuda.synchronize()
    return diag


def jacobi_minv(entry, like: DeviceField, bounds: Box, others: Sequence[DeviceField] = (), reach=None,
                region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None) -> DeviceField:
    """the Jacobi preconditioner of a linear operator for cg_solve(minv=...): 1 / diagonal (one division in the element
    type) on Omega, 1 elsewhere; arguments as operator_diagonal.  ValueError when a diagonal entry on Omega is 0 or not
    finite.  (A negative entry is not refused here: the solver wants a positive preconditioner and does not check.)"""
    import torch
    diag = operator_diagonal(entry, like, bounds, others, reach, region, cfg)
    lo, hi = _omega(like, bounds, region)
    minv = DeviceField.empty_like(like)
    minv.tensor.fill_(1.0)
    if any(h <= l for l, h in zip(lo, hi)):
        return minv
    cells = tuple(slice(l, h) for l, h in zip(lo, hi))
    d = diag.tensor[cells]
    bad = int(((d == 0) | ~torch.isfinite(d)).sum().item())
    if bad:
        raise ValueError(f"jacobi_minv: {bad} diagonal entries on Omega are 0 or not finite")
    minv.tensor[cells] = torch.ones_like(d) / d
    return minv


def _as_field(x) -> DeviceField:
    """a DeviceField as it is; a contiguous torch CUDA tensor as a field with a zero-based box"""
    if isinstance(x, DeviceField):
        return x
    import torch
    dtype = {torch.float64: _capi.F64, torch.float32: _capi.F32}[x.dtype]
    return DeviceField((0,) * x.dim(), tuple(x.shape), dtype, x)


def leapfrog_launch_counts():
    """(single launches, pair launches) of the last step_loop_leapfrog call, replays of its cached graph included"""
    singles, pairs = C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_leapfrog_launch_counts(C.byref(singles), C.byref(pairs))
    return singles.value, pairs.value


def group_launch_counts():
    """(groups of sibling applies run as ONE multi-output launch, member applies of a group run as launches of their
    own) since the process started"""
    fused, single = C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_group_launch_counts(C.byref(fused), C.byref(single))
    return fused.value, single.value


def step_loop_leapfrog(entry, geom, fields: Sequence, extra: Sequence = (), steps: int = 0,
                       cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None):
    """`steps` steps of the two-level scheme u(n+1) = F(u(n), u(n-1), extra...) that `entry` computes (a lowered apply's
    geometry-level entry whose inputs are: state, previous state, extra...), on rotating fields (torch CUDA tensors or
    DeviceFields): fields[0] = u(0), fields[1] = u(-1), fields[2] = scratch, and optionally fields[3] = a second scratch,
    which lets the loop take two steps per pass over HBM where the entry has a pair form (GeomEntry.fn_leapfrog2) and
    pairs measure faster.  `geom`: the apply's geometry (geom_for([u, u_prev, *extra], scratch, bounds)).  Long runs replay
    a cached hipGraph.  Asynchronous; -> (cur, prev): the indices into `fields` that hold u(steps) and u(steps - 1).
    leapfrog_launch_counts() tells which grouping ran."""
    lib = _capi.load()
    fs = [_as_field(f) for f in fields]
    ex = [_as_field(f) for f in extra]
    if len(fs) not in (3, 4):
        raise ValueError("step_loop_leapfrog: three fields (single launches) or four (pairs)")
    farr = (C.c_void_p * 4)(*([f.ptr for f in fs] + [None] * (4 - len(fs))))
    earr = (C.c_void_p * max(len(ex), 1))(*[f.ptr for f in ex])
    st = current_stream_ptr() if stream is None else stream
    fn2 = getattr(entry, "fn_leapfrog2", None)
    cur, prev = C.c_int(0), C.c_int(1)
    rc = lib.neptune_hip_step_loop_leapfrog(C.cast(entry.fn, C.c_void_p), C.cast(fn2, C.c_void_p) if fn2 is not None else None,
                                            C.byref(geom), farr, earr, len(ex), steps, st,
                                            C.byref(cfg) if cfg is not None else None, C.byref(cur), C.byref(prev))
    _capi.check(rc, "neptune_hip_step_loop_leapfrog")
    return cur.value, prev.value


def apply_group(entry, inputs: Sequence, outs: Sequence, bounds: Box, region: Optional[Box] = None,
                cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None) -> None:
    """outs[m] = member m's apply over `inputs` {bounds}, for every member of the group `entry`
    (LoweredModule.group_entry) in one call -- one multi-output launch where the group has that form.  `inputs`: the
    group's union inputs in the order of entry.inputs; DeviceFields or torch CUDA tensors.  Asynchronous on `stream`."""
    ins, os_ = [_as_field(f) for f in inputs], [_as_field(f) for f in outs]
    if len(ins) != entry.num_inputs or len(os_) != entry.num_outputs:
        raise ValueError(f"{entry.symbol}: {entry.num_inputs} inputs and {entry.num_outputs} results")
    g = geom_for(ins, os_[0], bounds, region)
    st = current_stream_ptr() if stream is None else stream
    _capi.check(entry(g, _in_array(ins), _in_array(os_), st, cfg), entry.symbol)


def system_loop_counts():
    """(steps issued or replayed, hipGraphLaunch calls that carried them) of the last step_loop_system call"""
    launches, graphs = C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_system_loop_counts(C.byref(launches), C.byref(graphs))
    return launches.value, graphs.value


def step_loop_system(entry, bounds: Box, cur: Sequence, nxt: Sequence, fixed: Sequence = (), steps: int = 0,
                     cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None):
    """`steps` steps of the system that the group `entry` (LoweredModule.group_entry) computes: member m advances the
    unknown in cur[m] (DeviceFields or torch CUDA tensors, in member order), nxt[m] is that unknown's second buffer; step s
    reads one set and writes the other.  `fixed`: the group's union inputs that are nobody's unknown (coefficient fields),
    in the order they have in entry.inputs.  Long runs replay a cached hipGraph.  Asynchronous; returns whichever of `cur`
    and `nxt` holds the newest state -- the other one then holds the state one step earlier."""
    lib = _capi.load()
    a, b, fx = [_as_field(f) for f in cur], [_as_field(f) for f in nxt], [_as_field(f) for f in fixed]
    n = entry.num_outputs
    fixed_slots = [k for k in range(entry.num_inputs) if k not in entry.through]
    if len(a) != n or len(b) != n or len(fx) != len(fixed_slots):
        raise ValueError(f"{entry.symbol}: {n} unknowns in cur and in nxt, {len(fixed_slots)} fixed inputs")
    ins = [None] * entry.num_inputs
    for m, k in enumerate(entry.through):
        ins[k] = a[m]
    for f, k in zip(fx, fixed_slots):
        ins[k] = f
    g = geom_for(ins, b[0], bounds)
    in_arr = (C.c_void_p * entry.num_inputs)(*[ins[k].ptr if k in fixed_slots else None for k in range(entry.num_inputs)])
    st = current_stream_ptr() if stream is None else stream
    rc = lib.neptune_hip_step_loop_system(C.cast(entry.fn, C.c_void_p), C.byref(g), n, (C.c_int * n)(*entry.through),
                                          _in_array(a), _in_array(b), in_arr, steps, st,
                                          C.byref(cfg) if cfg is not None else None)
    _capi.check(rc, "neptune_hip_step_loop_system")
    return list(nxt) if steps % 2 else list(cur)


def apply_twice(body, inp: DeviceField, out: DeviceField, bounds: Box, region: Optional[Box] = None,
                cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None, applies: int = 2) -> bool:
    """out = A(A(inp)) -- or A(A(A(inp))) with applies=3 -- in ONE pass over HBM for apply A (a built-in body id or a
    lowered apply's geometry-level entry); returns False -- having launched nothing -- when the body or the geometry does
    not qualify."""
    lib = _capi.load()
    g = geom_for([inp], out, bounds, region)
    st = current_stream_ptr() if stream is None else stream
    cfg_p = C.byref(cfg) if cfg is not None else None
    if hasattr(body, "fn"):
        f = getattr(body, "fn2" if applies == 2 else "fn3", None)
        if f is None:
            return False
        rc = f(C.byref(g), _in_array([inp]), out.ptr, st, cfg_p)
        what = body.symbol + str(applies)
    else:
        rc = lib.neptune_hip_apply_chain_builtin(body, applies, C.byref(g), _in_array([inp]), out.ptr, st, cfg_p)
        what = "neptune_hip_apply_chain_builtin"
    if rc == _capi.EUNSUPPORTED:
        return False
    _capi.check(rc, what)
    return True


def plan_builtin(body: int, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box,
                 region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None) -> int:
    lib = _capi.load()
    g = geom_for(inputs, out, bounds, region)
    return _capi.check(lib.neptune_hip_apply_builtin_plan(body, C.byref(g), _in_array(inputs), out.ptr,
                                                          C.byref(cfg) if cfg is not None else None),
                       "neptune_hip_apply_builtin_plan")


def time_builtin(body, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box,
                 cfg: Optional[_capi.LaunchCfg] = None, warmup: int = 3, reps: int = 20,
                 stream: Optional[int] = None) -> float:
    """average milliseconds per launch, HIP events on the launch stream (blocking).  `body`: a built-in body id
    or a lowered apply's geometry-level entry (LoweredModule.geom_entry)."""
    lib = _capi.load()
    g = geom_for(inputs, out, bounds)
    st = current_stream_ptr() if stream is None else stream
    cfg_p = C.byref(cfg) if cfg is not None else None
    if hasattr(body, "fn"):
        what = "neptune_hip_time_apply_fn"
        ms = lib.neptune_hip_time_apply_fn(C.cast(body.fn, C.c_void_p), C.byref(g), _in_array(inputs), out.ptr, st, cfg_p,
                                           warmup, reps)
    else:
        what = "neptune_hip_time_apply_builtin"
        ms = lib.neptune_hip_time_apply_builtin(body, C.byref(g), _in_array(inputs), out.ptr, st, cfg_p, warmup, reps)
    if ms < 0:
        raise _capi.NeptuneHipError(int(ms), what)
    return ms


def store(src: DeviceField, dst: DeviceField, bounds: Optional[Box] = None, stream: Optional[int] = None) -> None:
    """neptune_ir.store %src to %dst {bounds?}  (DataflowLowering.cpp:165-220)"""
    lib = _capi.load()
    st = current_stream_ptr() if stream is None else stream
    if src.dtype != dst.dtype:
        raise ValueError("store: element types differ")
    if bounds is None:
        if src.shape != dst.shape:
            raise ValueError("store: shapes differ")
        _capi.check(lib.neptune_hip_store_full(src.dtype, src.ptr, dst.ptr, src.count, st), "neptune_hip_store_full")
        return
    r = src.rank
    arr = lambda v: (C.c_int64 * r)(*[int(x) for x in v])
    _capi.check(lib.neptune_hip_store_box(src.dtype, r, src.ptr, arr(src.lb), arr(src.ub), dst.ptr, arr(dst.lb),
                                          arr(dst.ub), arr(bounds[0]), arr(bounds[1]), st), "neptune_hip_store_box")


def count_mismatch(a: DeviceField, b: DeviceField) -> int:
    lib = _capi.load()
    if a.dtype != b.dtype or a.shape != b.shape:
        raise ValueError("count_mismatch: fields differ in type or shape")
    n = lib.neptune_hip_count_mismatch(a.dtype, a.ptr, b.ptr, a.count, current_stream_ptr())
    if n < 0:
        raise RuntimeError("neptune_hip_count_mismatch failed")
    return int(n)


def reduce_sum(src: DeviceField, bounds: Optional[Box] = None, stream: Optional[int] = None) -> float:
    """neptune_ir.reduce %src (in bounds)? {kind = "sum"}  (DataflowLowering.cpp:589-698); blocking"""
    lib = _capi.load()
    r = src.rank
    arr = lambda v: (C.c_int64 * r)(*[int(x) for x in v])
    out = C.c_double(0.0)
    rc = lib.neptune_hip_reduce_sum(src.dtype, r, src.ptr, arr(src.lb), arr(src.ub),
                                    arr(bounds[0]) if bounds is not None else None,
                                    arr(bounds[1]) if bounds is not None else None, C.byref(out),
                                    current_stream_ptr() if stream is None else stream)
    _capi.check(rc, "neptune_hip_reduce_sum")
    return out.value


def reduce(src: DeviceField, kind, bounds: Optional[Box] = None, stream: Optional[int] = None) -> float:
    """neptune_ir.reduce %src (in bounds)? {kind = "sum" | "max" | "min" | "l1" | "l2"}; blocking.  kind: the name, or a
    _capi.REDUCE_* value (| _capi.REDUCE_RAW: l2 without its sqrt).  The value is computed in the field's element type
    and comes back widened to a Python float: max / min fold with arith.maximumf / minimumf (NaN if any cell is NaN,
    -0 < +0; -inf / +inf over an empty box), l1 = sum |x| and l2 = sqrt(sum x*x) on the fixed tree of reduce_sum
    (+0 over an empty box); kind "sum" returns the bits of reduce_sum."""
    lib = _capi.load()
    if isinstance(kind, str):
        if kind not in _capi.REDUCE_KINDS:
            raise ValueError(f"unknown reduce kind {kind!r} (expected one of {', '.join(_capi.REDUCE_KINDS)})")
        kind = _capi.REDUCE_KINDS[kind]
    r = src.rank
    arr = lambda v: (C.c_int64 * r)(*[int(x) for x in v])
    out = C.c_double(0.0)
    rc = lib.neptune_hip_reduce(int(kind), src.dtype, r, src.ptr, arr(src.lb), arr(src.ub),
                                arr(bounds[0]) if bounds is not None else None,
                                arr(bounds[1]) if bounds is not None else None, C.byref(out),
                                current_stream_ptr() if stream is None else stream)
    _capi.check(rc, "neptune_hip_reduce")
    return out.value


def autotune_builtin(body, inputs: Sequence[DeviceField], out: DeviceField, bounds: Box,
                     region: Optional[Box] = None, reps: int = 5, stream: Optional[int] = None):
    """plan-time tuning: -> (LaunchCfg of the fastest tile/chunk for this geometry, its ms per launch).  `body`: a
    built-in body id (every tile of the library is a candidate) or a lowered apply's geometry-level entry (the tiles
    its module holds: GeomEntry.num_variants)."""
    lib = _capi.load()
    g = geom_for(inputs, out, bounds, region)
    best = _capi.LaunchCfg(0, -1, 0, 0)
    ms = C.c_double(0.0)
    st = current_stream_ptr() if stream is None else stream
    if hasattr(body, "fn"):
        rc = lib.neptune_hip_autotune_fn(C.cast(body.fn, C.c_void_p), body.num_variants, C.byref(g), _in_array(inputs),
                                         out.ptr, st, reps, C.byref(best), C.byref(ms))
        _capi.check(rc, "neptune_hip_autotune_fn")
    else:
        rc = lib.neptune_hip_autotune_builtin(body, C.byref(g), _in_array(inputs), out.ptr, st, reps, C.byref(best),
                                              C.byref(ms))
        _capi.check(rc, "neptune_hip_autotune_builtin")
    return best, ms.value
