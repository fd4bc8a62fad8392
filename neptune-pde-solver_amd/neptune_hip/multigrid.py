"""Geometric multigrid V-cycles on the device (neptune_hip_mg_solve): a hierarchy of applies -- one operator
per level shape --, damped-Jacobi smoothing, full-weighting restriction fused with the residual, and trilinear
prolongation, all in the element type with one rounding per operation.  The normative definition is in
include/neptune_hip.h; this module builds the C structs and allocates the work fields.

    levels = [multigrid.Level(entry_l, like_l, bounds_l, minv=multigrid.jacobi_weights(entry_l, like_l, bounds_l, omega=6 / 7))
              for ...]
    h = multigrid.Hierarchy(levels)
    cycles, rr0, rr_last, rr_checks = multigrid.solve(h, x, b, max_cycles=20, tol2=1e-16 * rr0)

multigrid.cg_solve(h, x, b, ...) wraps conjugate gradients around one symmetric V-cycle of the same hierarchy
(neptune_hip_mgcg_solve): the iteration count stays grid-independent where plain cycles stall, e.g. on
anisotropic operators.

Two neighbouring levels may coarsen only some dimensions and keep the others (semi-coarsening): the pair's
extents say which (m_fine = 2 m_coarse + 1 coarsened, m_fine = m_coarse kept).  coarsen_bounds(bounds, axes=...) gives the
next level's extents, Hierarchy.coarsened records what it found, and coarsening_plan(extents, weights) chooses the
dimensions per level for an axis-aligned anisotropic operator -sum_d w_d u_dd.

A level may smooth with line stages instead of the point sweep: Level(..., lines=[line_weights(entry, like,
bounds, axis=d, omega=0.8) for d in (0, 1)]) solves the operator's tridiagonal part along dimension 0, then along dimension
1, in every sweep -- the repair for anisotropy whose strong direction varies in space.  solve() then runs
neptune_hip_mg_solve_lines, and cg_solve(..., lines=True) wraps conjugate gradients around the line-smoothed cycle
(neptune_hip_mgcg_solve_lines): its iteration count does not move with the anisotropy.

multigrid.cg_solve_mixed(outer, inner, x, b, ...) is cg_solve in two precisions (neptune_hip_mgcg_solve_mixed):
x, b and the CG recurrences in float64 on the operator of the Level `outer`, the V-cycle of the preconditioner in float32 on
the Hierarchy `inner` -- the same iteration count at about 0.6 of the bytes per iteration.

Cell-centred grids: a pair of levels may instead halve dimensions, m_fine = 2 m_coarse -- the coarse cell j
covers the fine cells 2 j and 2 j + 1 --, with averaging restriction and piecewise-constant prolongation; the boundary
conditions live in the operator (e.g. face coefficients that vanish on a Neumann face).  coarsen_bounds(...,
centring="cell") and coarsening_plan(..., centring="cell") give the extents, Hierarchy.halved records what it found; one
pair is one grid kind (halved and coarsened dimensions do not mix in a pair; kept ones mix with either).  The pure-Neumann
problem is singular: b must sum to zero over Omega, and the mean of x is whatever the iteration leaves.

Linear prolongation on cell-centred pairs: Level(..., prolong="linear", faces="dirichlet" | "neumann" | one
(low, high) pair per dimension) interpolates with the weights 3/4 and 1/4 and the stated rule per face; plain cycles
(solve) are then grid-independent where the constant prolongation is not.  The cycle is no longer a symmetric
preconditioner: cg_solve and cg_solve_mixed refuse such a hierarchy.

Transposed linear restriction: Level(..., prolong="linear", faces=..., restrict="linear") restricts by the
transpose of that prolongation under the same face rules, R = P^T / 2^k.  The pair is symmetric again, so cg_solve,
cg_solve(..., lines=True) and cg_solve_mixed accept it (Hierarchy.symmetric) and keep a grid-independent iteration count
on Dirichlet faces, where the constant pair does not.  For plain cycles the linear / averaging pair stays the better one.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

from . import _capi
from . import apply as _apply
from .fields import DeviceField, current_stream_ptr
from .geometry import Box, make_geom


def _centring(name: str, centring) -> bool:
    """-> whether `centring` is "cell"; ValueError unless it is "vertex" or "cell"."""
    if centring not in ("vertex", "cell"):
        raise ValueError(f'{name}: centring is "vertex" or "cell", not {centring!r}')
    return centring == "cell"


def coarsen_bounds(bounds: Box, axes=None, centring: str = "vertex") -> list:
    """the next level's interior extents for a level whose interior is `bounds` (lb, ub): (m - 1) / 2 along every dimension
    in `axes` (an iterable of dimensions to coarsen; default: all of them), m itself along the others (kept: semi-coarsening,
    DESIGN 3.16).  ValueError when a coarsened extent is even (a vertex-centred grid with a Dirichlet rim nests only for odd
    extents) or below 3 -- a kept one may be anything --, when `axes` is empty or names a dimension the bounds do not have.
    centring="cell" (DESIGN 3.20): m / 2 along every dimension in `axes` (halved); ValueError for an odd extent or one
    below 2."""
    cell = _centring("coarsen_bounds", centring)
    rank = len(bounds[0])
    chosen = set(range(rank)) if axes is None else {int(d) for d in axes}
    if not chosen:
        raise ValueError("coarsen_bounds: no dimension to coarsen (axes is empty)")
    if not chosen <= set(range(rank)):
        raise ValueError(f"coarsen_bounds: axes {sorted(chosen)} name a dimension outside 0..{rank - 1}")
    out = []
    for d, (l, u) in enumerate(zip(bounds[0], bounds[1])):
        m = int(u) - int(l)
        if d not in chosen:
            out.append(m)
            continue
        if cell:
            if m < 2 or m % 2 == 1:
                raise ValueError(f"coarsen_bounds: interior extent {m} of dimension {d} is not an even number >= 2")
            out.append(m // 2)
            continue
        if m < 3 or m % 2 == 0:
            raise ValueError(f"coarsen_bounds: interior extent {m} of dimension {d} is not an odd number >= 3")
        out.append((m - 1) // 2)
    return out


def coarsening_plan(extents, weights, threshold: float = 0.5, max_levels: int = 16, centring: str = "vertex") -> list:
    """which dimensions to coarsen on each level of a hierarchy for the operator  -sum_d w_d u_dd  on unscaled star stencils
    with rscale = 4; -> per level (extents, weights, axes), finest first, `axes` = the dimensions coarsened
    towards the next level (() on the last).

    The rule: a dimension is coarsenable when its extent is odd and >= 3; of those, the ones whose weight is at least
    `threshold` x the largest weight among them are coarsened -- the smoother smooths along strongly coupled dimensions
    only.  The next level keeps w_d on a coarsened dimension and takes 4 w_d on a kept one (with rscale = 4 the coarse
    stencil is the fine one's, so relative to the coarsened dimensions, whose spacing doubled, a kept one couples 4x as
    strongly): the anisotropy falls 4x per level until every dimension is coarsened.  The plan ends when nothing is
    coarsenable or after max_levels levels.

    A heuristic for axis-aligned anisotropy -- one constant weight per dimension --, not a general coarsening strategy:
    it knows nothing of variable coefficients, rotated anisotropy or mixed derivatives.

    centring="cell" (DESIGN 3.20): a dimension is coarsenable when its extent is even and >= 4 and is halved, m / 2; the
    rule is otherwise the same.  An extent ends at 2: a Neumann level of extent 1 has a zero diagonal and cannot be
    smoothed."""
    cell = _centring("coarsening_plan", centring)
    m = [int(v) for v in extents]
    w = [float(v) for v in weights]
    if len(m) != len(w) or not m or any(v < 1 for v in m) or any(not v > 0.0 for v in w):
        raise ValueError("coarsening_plan: one positive weight per dimension, extents >= 1")
    plan = []
    while True:
        can = [d for d, v in enumerate(m) if (v >= 4 and v % 2 == 0 if cell else v >= 3 and v % 2 == 1)]
        if not can or len(plan) + 1 >= max_levels:
            plan.append((tuple(m), tuple(w), ()))
            return plan
        strongest = max(w[d] for d in can)
        axes = tuple(d for d in can if w[d] >= threshold * strongest)
        plan.append((tuple(m), tuple(w), axes))
        m = [(v // 2 if cell else (v - 1) // 2) if d in axes else v for d, v in enumerate(m)]
        w = [v if d in axes else 4.0 * v for d, v in enumerate(w)]


def jacobi_weights(entry, like: DeviceField, bounds: Box, others: Sequence[DeviceField] = (), omega: float = 1.0, reach=None,
                   region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None) -> DeviceField:
    """the damped-Jacobi weights of a linear operator for Level(minv=...): omega / diagonal (one division in the element
    type) on Omega = bounds x region, +0 elsewhere; the other arguments as apply.operator_diagonal, on which it is built.
    ValueError when a diagonal entry on Omega is 0 or not finite (as apply.jacobi_minv)."""
    import torch
    diag = _apply.operator_diagonal(entry, like, bounds, others, reach, region, cfg)
    lo, hi = _apply._omega(like, bounds, region)
    w = DeviceField.empty_like(like)
    w.tensor.zero_()
    if any(h <= l for l, h in zip(lo, hi)):
        return w
    cells = tuple(slice(l, h) for l, h in zip(lo, hi))
    d = diag.tensor[cells]
    bad = int(((d == 0) | ~torch.isfinite(d)).sum().item())
    if bad:
        raise ValueError(f"jacobi_weights: {bad} diagonal entries on Omega are 0 or not finite")
    w.tensor[cells] = torch.full_like(d, float(omega)) / d
    return w


def operator_tridiagonal(entry, like: DeviceField, bounds: Box, axis: int, others: Sequence[DeviceField] = (), reach=None,
                         region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None):
    """the tridiagonal part of a LINEAR operator along dimension `axis`, restricted to Omega = bounds x region:
    -> (lower, diag, upper), fields like `like` with A's entry at (p, p - e_axis), (p, p), (p, p + e_axis) on the cells p of
    Omega and +0 elsewhere; an entry that couples to a cell outside Omega (the rim) is +0.  The coloured unit-vector probes of
    apply.operator_diagonal, with its guard launch, its arguments and its caveat for an affine operator: with a colour at
    cell j the result at j - e_axis is `upper` of that cell and the result at j + e_axis is `lower` of that cell -- cells of
    one colour are 2 reach + 1 >= 3 apart along `axis`, so neither sees another coloured cell.  ValueError when reach along
    `axis` is below 1.  Set-up work, blocking."""
    import itertools
    import torch
    axis = int(axis)
    if not 0 <= axis < like.rank:
        raise ValueError(f"operator_tridiagonal: axis {axis} is outside 0..{like.rank - 1}")
    if reach is None:
        if not hasattr(entry, "halo0"):
            raise ValueError("operator_tridiagonal: reach is required for a built-in body")
        reach = entry.halo0
    reach = [int(reach)] * like.rank if isinstance(reach, int) else [int(r) for r in reach]
    if len(reach) != like.rank or any(r < 0 for r in reach):
        raise ValueError("operator_tridiagonal: reach is a non-negative int or one per dimension")
    if reach[axis] < 1:
        raise ValueError(f"operator_tridiagonal: reach along axis {axis} must be at least 1")
    others = list(others)
    lo, hi = _apply._omega(like, bounds, region)
    lower, diag, upper = (DeviceField.empty_like(like) for _ in range(3))
    for f in (lower, diag, upper):
        f.tensor.zero_()
    if any(h <= l for l, h in zip(lo, hi)):
        return lower, diag, upper
    probe, out = DeviceField.empty_like(like), DeviceField.empty_like(like)
    stride = [2 * r + 1 for r in reach]
    mid = [(l + h) // 2 for l, h in zip(lo, hi)]
    probe.tensor.zero_()
    probe.tensor[tuple(mid)] = 1.0
    out.tensor.zero_()
    _apply.apply_builtin(entry, [probe] + others, out, bounds, region=region, cfg=cfg)
    seen = out.tensor[tuple(slice(l, h) for l, h in zip(lo, hi))].clone()
    seen[tuple(slice(max(m - r - l, 0), m + r + 1 - l) for m, r, l in zip(mid, reach, lo))] = 0.0
    if bool((seen != 0).any()):
        raise ValueError(f"operator_tridiagonal: the operator reaches further than reach = {reach} (a unit vector at {mid} is "
                         "seen beyond it): give reach per dimension")
    for colour in itertools.product(*[range(min(s, h - l)) for s, l, h in zip(stride, lo, hi)]):
        cells = [slice(l + c, h, s) for l, h, c, s in zip(lo, hi, colour, stride)]
        probe.tensor.zero_()
        probe.tensor[tuple(cells)] = 1.0
        out.tensor.zero_()
        _apply.apply_builtin(entry, [probe] + others, out, bounds, region=region, cfg=cfg)
        diag.tensor[tuple(cells)] = out.tensor[tuple(cells)]
        l, h, c, s = lo[axis], hi[axis], colour[axis], stride[axis]
        below, above = list(cells), list(cells)
        below[axis] = slice(l + c - 1 if c >= 1 else l + c + s - 1, h - 1, s)   # j - 1 for the coloured j >= l + 1
        above[axis] = slice(l + c + 1, h, s)                                    # j + 1 for the coloured j <= h - 2
        upper.tensor[tuple(below)] = out.tensor[tuple(below)]
        lower.tensor[tuple(above)] = out.tensor[tuple(above)]
    torch.cuda.synchronize()
    return lower, diag, upper


class LineStage(NamedTuple):
    """one stage of a line smoother: the field dimension the lines run along and the factor fields of Thomas's elimination
    (line_weights; the definition is in include/neptune_hip.h)"""
    axis: int
    lo: DeviceField
    inv: DeviceField
    up: DeviceField


def line_factors(lower, diag, upper, where, axis: int, omega: float = 1.0):
    """the factor recurrence of a line stage on NumPy arrays (the tridiagonal part of the operator over the level's box,
    `where`: Omega as a tuple of slices): -> (lo, inv, up), in the arrays' element type with one rounding per operation, +0
    outside Omega; ValueError when a pivot is 0 or not finite"""
    import numpy as np
    dt = diag.dtype.type
    w = dt(omega)
    move = lambda a: np.moveaxis(a[where], axis, 0)
    l, t, u = move(lower), move(diag), move(upper)
    m = t.shape[0]
    lo_, inv_, up_ = (np.zeros(t.shape, diag.dtype) for _ in range(3))
    with np.errstate(all="ignore"):
        ls, ts, us = (l / w).astype(dt), (t / w).astype(dt), (u / w).astype(dt)
        c = None
        for i in range(m):
            if i == 0:
                den = ts[0]
            else:
                p = (ls[i] * c).astype(dt)
                den = (ts[i] - p).astype(dt)
            bad = int(((den == 0) | ~np.isfinite(den)).sum())
            if bad:
                raise ValueError(f"line_weights: {bad} pivots at interior index {i} along axis {axis} are 0 or not finite")
            inv_[i] = (dt(1) / den).astype(dt)
            c = (us[i] * inv_[i]).astype(dt)
            if i > 0:
                lo_[i] = ls[i]
            if i < m - 1:
                up_[i] = c
    out = []
    for a in (lo_, inv_, up_):
        full = np.zeros(diag.shape, diag.dtype)
        full[where] = np.moveaxis(a, 0, axis)
        out.append(full)
    return tuple(out)


def line_weights(entry, like: DeviceField, bounds: Box, axis: int, others: Sequence[DeviceField] = (), omega: float = 1.0,
                 reach=None, region: Optional[Box] = None, cfg: Optional[_capi.LaunchCfg] = None) -> LineStage:
    """the factors of a line stage along dimension `axis` for Level(lines=...): Thomas's elimination of T / omega, T the
    tridiagonal part of the operator along `axis` restricted to Omega (operator_tridiagonal, whose arguments the others are).
    The recurrence is set-up work and runs on the host in NumPy, in the element type with one rounding per operation as
    include/neptune_hip.h defines it -- the device's division is not relied on.  ValueError when a pivot (t'_0 or a den) is 0
    or not finite."""
    lower, diag, upper = operator_tridiagonal(entry, like, bounds, axis, others, reach, region, cfg)
    lo, hi = _apply._omega(like, bounds, region)
    where = tuple(slice(l, h) for l, h in zip(lo, hi))
    if any(h <= l for l, h in zip(lo, hi)):
        return LineStage(int(axis), lower, diag, upper)   # all +0
    f = line_factors(lower.numpy(), diag.numpy(), upper.numpy(), where, int(axis), omega)
    return LineStage(int(axis), *[DeviceField.from_numpy(a) for a in f])


class Level:
    """one level of a hierarchy: the operator (`entry`: a built-in body id or a lowered apply's geometry-level entry whose
    input 0 has the result's box), a field `like` that gives the level's box and element type, the apply's `bounds`
    (logical), its fixed inputs 1.. (`others`), the smoother's weights `minv` (a field like `like`: omega / diagonal on
    Omega, e.g. jacobi_weights; required before a solve), the factor `rscale` of the restriction that leaves this level
    (4 for an operator that is not scaled by 1 / h^2: the coarse operator is then the fine one's stencil), the launch
    `region` (result-physical, default: the whole box) and `lines`: up to three LineStages (line_weights) that replace the
    point sweep on this level; minv may be omitted when lines is given.
    prolong, faces describe the prolongation of the pair that LEAVES this level (ignored on the last one): "constant", what
    the pair's grid kind implies, or "linear" (a cell-centred pair only), which needs the rule per face:
    faces = "neumann" or "dirichlet" (the value 0 on the face) for all faces, or one (low, high) pair of these per
    dimension.  restrict describes the restriction of the same pair: "average", what the pair's grid kind implies, or
    "linear" (a cell-centred pair only): the transpose of the linear prolongation by the same `faces`.
    Hierarchy checks all three."""

    def __init__(self, entry, like: DeviceField, bounds: Box, others: Sequence[DeviceField] = (), minv: Optional[DeviceField] = None,
                 rscale: float = 4.0, region: Optional[Box] = None, lines: Sequence[LineStage] = (), prolong: str = "constant",
                 faces=None, restrict: str = "average"):
        self.prolong, self.faces, self.restrict = prolong, faces, restrict
        self.lines = [LineStage(*st) for st in lines]
        if len(self.lines) > 3:
            raise ValueError("Level: at most three line stages")
        for st in self.lines:
            if not 0 <= int(st.axis) < like.rank:
                raise ValueError(f"Level: a line stage along axis {st.axis} on a field of rank {like.rank}")
            if any(f.box != like.box or f.dtype != like.dtype for f in (st.lo, st.inv, st.up)):
                raise ValueError("Level: a line stage's factor fields must have the box and the element type of `like`")
        self.entry, self.like, self.others, self.minv, self.rscale, self.region = entry, like, list(others), minv, float(rscale), region
        self.bounds = ([int(v) for v in bounds[0]], [int(v) for v in bounds[1]])
        self.geom = make_geom(like.box, self.bounds, [like.box] + [f.box for f in self.others], region)
        self.lo, self.hi = _apply._omega(like, self.bounds, region)
        self.m = [h - l for l, h in zip(self.lo, self.hi)]
        if minv is not None and (minv.box != like.box or minv.dtype != like.dtype):
            raise ValueError("Level: minv must have the box and the element type of `like`")

    @property
    def omega(self):
        """numpy / torch index of Omega in the level's fields"""
        return tuple(slice(l, h) for l, h in zip(self.lo, self.hi))

    @property
    def linear(self) -> bool:
        return self.prolong == "linear"

    @property
    def restrict_linear(self) -> bool:
        return self.restrict == "linear"

    def transfer_struct(self) -> _capi.MgTransfer:
        """neptune_hip_mg_transfer_t of the pair that leaves this level; ValueError for a malformed prolong / restrict / faces"""
        t = _capi.MgTransfer()
        if self.prolong not in ("constant", "linear"):
            raise ValueError(f'prolong is "constant" or "linear", not {self.prolong!r}')
        if self.restrict not in ("average", "linear"):
            raise ValueError(f'restrict is "average" or "linear", not {self.restrict!r}')
        t.prolong = _capi.MG_PROLONG_LINEAR if self.linear else _capi.MG_PROLONG_CONSTANT
        t.restrict_kind = _capi.MG_RESTRICT_LINEAR if self.restrict_linear else _capi.MG_RESTRICT_AVERAGE
        if self.linear or self.restrict_linear:
            lo, hi = face_rules(self.faces, self.like.rank, "restrict" if not self.linear else "prolong")
            for d in range(self.like.rank):
                t.rim_lo[d], t.rim_hi[d] = lo[d], hi[d]
        return t

    def prolong_struct(self) -> _capi.MgProlong:
        """neptune_hip_mg_prolong_t of the pair that leaves this level; ValueError for a malformed prolong / faces"""
        p = _capi.MgProlong()
        if self.prolong not in ("constant", "linear"):
            raise ValueError(f'prolong is "constant" or "linear", not {self.prolong!r}')
        if not self.linear:
            p.kind = _capi.MG_PROLONG_CONSTANT
            return p
        p.kind = _capi.MG_PROLONG_LINEAR
        lo, hi = face_rules(self.faces, self.like.rank)
        for d in range(self.like.rank):
            p.rim_lo[d], p.rim_hi[d] = lo[d], hi[d]
        return p


_FACE_RULE = {"neumann": _capi.MG_RIM_EVEN, "dirichlet": _capi.MG_RIM_ODD}


def face_rules(faces, rank: int, what: str = "prolong"):
    """the linear prolongation's rule per face from `faces`: "neumann" / "dirichlet" for all faces, or a
    sequence of `rank` (low, high) pairs of them; -> (low rules, high rules) per dimension as _capi.MG_RIM_EVEN / _ODD;
    ValueError for anything else"""
    if faces is None:
        raise ValueError(f'{what}="linear" needs faces ("neumann", "dirichlet", or a (low, high) pair of them per dimension)')
    if isinstance(faces, str):
        faces = [(faces, faces)] * rank
    try:
        pairs = [tuple(f) for f in faces]
    except TypeError:
        pairs = None
    if (pairs is None or len(pairs) != rank or any(len(f) != 2 or isinstance(f, str) for f in faces)
            or any(not isinstance(v, str) or v not in _FACE_RULE for f in pairs for v in f)):
        raise ValueError(f'faces is "neumann", "dirichlet", or {rank} (low, high) pairs of them (one per dimension), not {faces!r}')
    return [_FACE_RULE[f[0]] for f in pairs], [_FACE_RULE[f[1]] for f in pairs]


def _fill_level(struct, L: Level, x: DeviceField, b: DeviceField, q: DeviceField, keep: list) -> None:
    """the operator of level L and its fields x, b, q into one neptune_hip_mg_level_t (all but minv); what must stay alive
    while the struct is used is appended to `keep`"""
    is_entry = hasattr(L.entry, "fn")
    struct.fn = C.cast(L.entry.fn, C.c_void_p) if is_entry else None
    struct.body = -1 if is_entry else int(L.entry)
    struct.g = L.geom
    if L.others:
        rest = (C.c_void_p * len(L.others))(*[f.ptr for f in L.others])
        keep.append(rest)
        struct.in_rest = rest
    struct.x, struct.b, struct.q, struct.rscale = x.ptr, b.ptr, q.ptr, L.rscale


class Hierarchy:
    """the levels of a solve, finest first.  Checks the size relation per dimension -- coarsened, m_l = 2 m_(l+1) + 1, or
    kept, m_l = m_(l+1); at least one coarsened -- (ValueError naming the level and the dimension), one rank and one
    element type; allocates x_l and b_l for l >= 1 and every q_l.  coarsened[l]: the tuple of dimensions coarsened between
    level l and l + 1.  A pair may instead be cell-centred: dimensions halved, m_l = 2 m_(l+1), the others
    kept; halved[l]: the tuple of dimensions halved between level l and l + 1 (() for a vertex-centred pair), and
    coarsened[l] then lists the same dimensions, as neptune_hip_mg_coarsened_axes does.  A pair with both a coarsened and
    a halved dimension is refused (ValueError naming the level and both kinds)."""

    def __init__(self, levels: Sequence[Level]):
        self.levels = list(levels)
        if not 1 <= len(self.levels) <= 16:
            raise ValueError("Hierarchy: 1..16 levels")
        first = self.levels[0]
        self.coarsened = []
        self.halved = []
        for l, L in enumerate(self.levels):
            if L.like.rank != first.like.rank or L.like.dtype != first.like.dtype:
                raise ValueError(f"Hierarchy: level {l} has another rank or element type than level 0")
            if any(m < 1 for m in L.m):
                raise ValueError(f"Hierarchy: level {l} has an empty Omega")
            if l > 0:
                axes, halved = [], []
                for d, (mf, mc) in enumerate(zip(self.levels[l - 1].m, L.m)):
                    if mf == 2 * mc + 1:
                        axes.append(d)
                    elif mf == 2 * mc:
                        halved.append(d)
                    elif mf != mc:
                        raise ValueError(f"Hierarchy: level {l}, dimension {d}: interior extent {mc} does not nest in level "
                                         f"{l - 1}'s {mf} (m_fine = 2 m_coarse + 1, or m_fine = m_coarse for a kept dimension)")
                if axes and halved:
                    raise ValueError(f"Hierarchy: level {l} mixes two grid kinds against level {l - 1}: dimensions {axes} are "
                                     f"coarsened (vertex-centred, m_fine = 2 m_coarse + 1) and dimensions {halved} are halved "
                                     "(cell-centred, m_fine = 2 m_coarse); one pair of levels is one grid kind")
                if not axes and not halved:
                    raise ValueError(f"Hierarchy: level {l} coarsens no dimension of level {l - 1}")
                self.coarsened.append(tuple(axes or halved))
                self.halved.append(tuple(halved))
                above = self.levels[l - 1]
                try:
                    above.prolong_struct()
                    above.transfer_struct()
                except ValueError as err:
                    raise ValueError(f"Hierarchy: level {l - 1}: {err}") from None
                if above.restrict_linear and not halved:
                    raise ValueError(f'Hierarchy: level {l - 1}: restrict="linear" needs a cell-centred pair, but no dimension is '
                                     f"halved towards level {l} (m_fine = 2 m_coarse)")
                if above.linear and not halved:
                    raise ValueError(f'Hierarchy: level {l - 1}: prolong="linear" needs a cell-centred pair, but no dimension is '
                                     f"halved towards level {l} (m_fine = 2 m_coarse)")
        self.dtype, self.rank = first.like.dtype, first.like.rank
        self.q = [DeviceField.empty_like(L.like) for L in self.levels]
        self.x = [None] + [DeviceField.empty_like(L.like) for L in self.levels[1:]]
        self.b = [None] + [DeviceField.empty_like(L.like) for L in self.levels[1:]]

    def __len__(self):
        return len(self.levels)

    def _structs(self, x: DeviceField, b: DeviceField):
        """-> (the C array of levels, what must stay alive while it is used)"""
        n = len(self.levels)
        arr = (_capi.MgLevel * n)()
        keep = []
        for l, L in enumerate(self.levels):
            if L.minv is None and not L.lines:
                raise ValueError(f"multigrid: level {l} has no minv (jacobi_weights) and no line stages")
            _fill_level(arr[l], L, x if l == 0 else self.x[l], b if l == 0 else self.b[l], self.q[l], keep)
            arr[l].minv = L.minv.ptr if L.minv is not None else None
        return arr, keep

    @property
    def has_lines(self) -> bool:
        return any(L.lines for L in self.levels)

    @property
    def has_linear(self) -> bool:
        """whether any pair of levels prolongs linearly (the last level's setting is ignored)"""
        return any(L.linear for L in self.levels[:-1])

    @property
    def has_linear_restrict(self) -> bool:
        """whether any pair of levels restricts by the transposed linear prolongation"""
        return any(L.restrict_linear for L in self.levels[:-1])

    @property
    def symmetric(self) -> bool:
        """whether every pair's prolongation is a multiple of its restriction's transpose, so that a V(s, s) cycle is a symmetric
        preconditioner: each pair is constant / average or linear / linear (the last level's settings are ignored)"""
        return all(L.linear == L.restrict_linear for L in self.levels[:-1])

    def _transfer_structs(self):
        """-> the C array of neptune_hip_mg_transfer_t, entry l for the pair (l, l + 1)"""
        arr = (_capi.MgTransfer * max(len(self.levels) - 1, 1))()
        for l, L in enumerate(self.levels[:-1]):
            arr[l] = L.transfer_struct()
        return arr

    def _prolong_structs(self):
        """-> the C array of neptune_hip_mg_prolong_t, entry l for the pair (l, l + 1)"""
        arr = (_capi.MgProlong * max(len(self.levels) - 1, 1))()
        for l, L in enumerate(self.levels[:-1]):
            arr[l] = L.prolong_struct()
        return arr

    def _line_structs(self):
        """-> the C array of neptune_hip_mg_lines_t, one per level (the factor fields stay alive in the levels)"""
        arr = (_capi.MgLines * len(self.levels))()
        for l, L in enumerate(self.levels):
            arr[l].n_stages = len(L.lines)
            for s, st in enumerate(L.lines):
                arr[l].axis[s] = int(st.axis)
                arr[l].lo[s], arr[l].inv[s], arr[l].up[s] = st.lo.ptr, st.inv.ptr, st.up.ptr
        return arr


def counts():
    """(cycles that ran as plain launches, cycles that ran as graph launches, read-backs after blocks of cycles) of the last
    solve call"""
    plain, graph, checks = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _capi.load().neptune_hip_mg_counts(C.byref(plain), C.byref(graph), C.byref(checks))
    return plain.value, graph.value, checks.value


def solve(h: Hierarchy, x: DeviceField, b: DeviceField, pre: int = 2, post: int = 2, coarse_sweeps: int = 8, max_cycles: int = 20,
          tol2: float = 0.0, check_every: int = 1, cfg: Optional[_capi.LaunchCfg] = None, stream: Optional[int] = None):
    """solve A_0(x) = b by V(pre, post) cycles over the hierarchy `h` (neptune_hip_mg_solve; neptune_hip_mg_solve_lines when
    any level has line stages; neptune_hip_mg_solve_prolong when any pair prolongs linearly; neptune_hip_mg_solve_transfer when
    any pair restricts by the transposed linear prolongation).  x: initial guess in, solution
    out; its cells outside Omega_0 are boundary data and are never written.  The loop stops when r . r <= tol2 (checked every
    `check_every` cycles) or after max_cycles cycles.  cfg: the launch configuration of level 0's operator.
    Blocking; -> (cycles, rr0, rr_last, rr_checks): rr_checks is the list of r . r values read after each block of cycles.
    counts() tells how the cycles were launched."""
    lib = _capi.load()
    first = h.levels[0].like
    if x.box != first.box or b.box != first.box or x.dtype != h.dtype or b.dtype != h.dtype:
        raise ValueError("multigrid.solve: x and b must have the box and the element type of level 0")
    arr, keep = h._structs(x, b)
    st = current_stream_ptr() if stream is None else stream
    n_checks = max(-(-int(max_cycles) // max(int(check_every), 1)), 1)
    rr = (C.c_double * n_checks)()
    done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    rest = (pre, post, coarse_sweeps, max_cycles, check_every, tol2, rr, st, C.byref(cfg) if cfg is not None else None,
            C.byref(done), C.byref(rr0), C.byref(last))
    if h.has_linear_restrict:
        _capi.check(lib.neptune_hip_mg_solve_transfer(arr, h._line_structs() if h.has_lines else None, h._transfer_structs(), len(h),
                                                      h.dtype, *rest), "neptune_hip_mg_solve_transfer")
    elif h.has_linear:
        _capi.check(lib.neptune_hip_mg_solve_prolong(arr, h._line_structs() if h.has_lines else None, h._prolong_structs(), len(h),
                                                     h.dtype, *rest), "neptune_hip_mg_solve_prolong")
    elif h.has_lines:
        _capi.check(lib.neptune_hip_mg_solve_lines(arr, h._line_structs(), len(h), h.dtype, *rest), "neptune_hip_mg_solve_lines")
    else:
        _capi.check(lib.neptune_hip_mg_solve(arr, len(h), h.dtype, *rest), "neptune_hip_mg_solve")
    del keep
    return done.value, rr0.value, last.value, list(rr[:counts()[2]])


_NOT_SYMMETRIC = ("multigrid.{}: the hierarchy has a pair with prolong=\"linear\" and the averaging restriction (or "
                  "restrict=\"linear\" and the constant prolongation): P is not a multiple of R^T, so the V-cycle would not be a "
                  "symmetric preconditioner and conjugate gradients do not apply; use multigrid.solve, or make the pair symmetric: "
                  "prolong=\"linear\" with restrict=\"linear\" (the transposed restriction, DESIGN 3.23), or prolong=\"constant\"")


def cg_counts():
    """(iterations that ran as plain launches, iterations that ran as graph launches, how many of all these took a plain
    launch and a separate dot product for q = A(p), read-backs after blocks of iterations) of the last cg_solve call"""
    vals = [C.c_int64(0) for _ in range(4)]
    _capi.load().neptune_hip_mgcg_counts(*[C.byref(v) for v in vals])
    return tuple(v.value for v in vals)


def cg_rz0() -> float:
    """r . M(r) after the set-up of the last cg_solve call (0 when it ran no iteration): with rr0 and the trace, every scalar
    the recurrences used"""
    return float(_capi.load().neptune_hip_mgcg_rz0())


def cg_solve(h: Hierarchy, x: DeviceField, b: DeviceField, sweeps: int = 2, coarse_sweeps: int = 8, max_iters: int = 50,
             tol2: float = 0.0, check_every: int = 1, trace: bool = False, dot="auto", cfg: Optional[_capi.LaunchCfg] = None,
             work: Optional[Sequence[DeviceField]] = None, stream: Optional[int] = None, lines: bool = False):
    """solve A_0(x) = b by conjugate gradients preconditioned with one V(sweeps, sweeps) cycle over the hierarchy `h`
    (neptune_hip_mgcg_solve; at least two levels, sweeps >= 1; every pair symmetric -- Hierarchy.symmetric --, a hierarchy with
    restrict="linear" pairs runs neptune_hip_mgcg_solve_transfer).  Level 0's minv must be finite on its whole box
    (jacobi_weights puts +0 outside Omega).  lines=True: a hierarchy whose levels have line stages runs
    neptune_hip_mgcg_solve_lines -- a level with stages needs no minv, level 0 included; without the keyword
    such a hierarchy is refused (ValueError).  A hierarchy without stages behaves the same either way.  x: initial guess in, solution out; its cells outside Omega_0 are boundary data
    and are never changed.  The loop stops when r . r <= tol2 (checked every `check_every` iterations) or after max_iters
    iterations.  dot: level 0's dot entry (LoweredModule.dot_entry), "auto": level 0's entry's own if it has one (built-in
    bodies do), "fallback" or None: a plain launch and a separate dot product per iteration.  work: three fields like x for
    r, p, z (allocated here when None).  cfg: the launch configuration of level 0's operator.
    Blocking; -> (iters, rr0, rr_last), and with trace=True a fourth item: a numpy array of shape (iters, 3) holding
    (p . A(p) of iteration k, r . M(r) after it, r . r after it).  cg_counts() tells how the iterations were launched."""
    lib = _capi.load()
    first = h.levels[0].like
    if x.box != first.box or b.box != first.box or x.dtype != h.dtype or b.dtype != h.dtype:
        raise ValueError("multigrid.cg_solve: x and b must have the box and the element type of level 0")
    if len(h) < 2:
        raise ValueError("multigrid.cg_solve: at least two levels (one level is apply.cg_solve with minv)")
    if not h.symmetric:
        raise ValueError(_NOT_SYMMETRIC.format("cg_solve"))
    if h.has_lines and not lines:
        raise ValueError("multigrid.cg_solve: the hierarchy has line stages; neptune_hip_mgcg_solve smooths with point Jacobi "
                         "only (its fused first and last sweeps on level 0): pass lines=True for neptune_hip_mgcg_solve_lines")
    if work is None:
        work = [DeviceField.empty_like(x) for _ in range(3)]
    fn_dot = _apply.resolve_dot("multigrid.cg_solve", h.levels[0].entry, dot)
    arr, keep = h._structs(x, b)
    st = current_stream_ptr() if stream is None else stream
    tr = _apply.trace_buffer(3, max_iters, x.tensor) if trace else None
    warr = (C.c_void_p * 3)(*[f.ptr for f in work])
    done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    rest = (fn_dot, sweeps, coarse_sweeps, warr, max_iters, check_every, tol2, tr.data_ptr() if trace else None, st,
            C.byref(cfg) if cfg is not None else None, C.byref(done), C.byref(rr0), C.byref(last))
    if h.has_linear_restrict:
        _capi.check(lib.neptune_hip_mgcg_solve_transfer(arr, h._line_structs() if h.has_lines else None, h._transfer_structs(), len(h),
                                                        h.dtype, *rest), "neptune_hip_mgcg_solve_transfer")
    elif h.has_lines:
        _capi.check(lib.neptune_hip_mgcg_solve_lines(arr, h._line_structs(), len(h), h.dtype, *rest), "neptune_hip_mgcg_solve_lines")
    else:
        _capi.check(lib.neptune_hip_mgcg_solve(arr, len(h), h.dtype, *rest), "neptune_hip_mgcg_solve")
    del keep
    if trace:
        return done.value, rr0.value, last.value, tr.cpu().numpy()[:3 * done.value].reshape(-1, 3)
    return done.value, rr0.value, last.value


def cg_solve_mixed(outer: Level, inner: Hierarchy, x: DeviceField, b: DeviceField, sweeps: int = 2, coarse_sweeps: int = 8,
                   max_iters: int = 50, tol2: float = 0.0, check_every: int = 1, trace: bool = False, dot="auto",
                   cfg: Optional[_capi.LaunchCfg] = None, work: Optional[Sequence[DeviceField]] = None, stream: Optional[int] = None):
    """solve A(x) = b in f64 by conjugate gradients whose preconditioner, one V(sweeps, sweeps) cycle, runs in f32
    (neptune_hip_mgcg_solve_mixed): x, b, r, p, q and every scalar stay f64, the cycle works on a narrowed copy
    of the residual, and the iteration count is that of cg_solve while the cycle moves half the bytes.  No scaling is
    applied: a residual that leaves f32's range must be scaled by the caller.
    outer: an f64 Level with the operator (entry, bounds, others, region); it needs no minv.  inner: an f32 Hierarchy of at
    least two levels whose level 0 has outer's box and Omega and its own f32 operator; levels >= 1 may have line stages,
    level 0 may not (ValueError).  The narrowed residual r32 and z32 are level 0's b and x: inner.b[0] and inner.x[0], f32
    fields allocated here when they are None and left there for the caller to read.  work: r, p and optionally q, f64 fields
    like x (allocated here when None).  dot: the outer operator's dot entry, as cg_solve's; cfg: the outer operator's launch
    configuration.  Everything else as cg_solve.
    Blocking; -> (iters, rr0, rr_last), and with trace=True a fourth item: a float64 numpy array of shape (iters, 3) holding
    (p . A(p) of iteration k, r32 . M32(r32) after it, r . r after it).  cg_counts() and cg_rz0() report on this call too."""
    import numpy as np
    import torch
    lib = _capi.load()
    first = inner.levels[0]
    if outer.like.dtype != _capi.F64 or x.dtype != _capi.F64 or b.dtype != _capi.F64:
        raise ValueError("multigrid.cg_solve_mixed: the outer level, x and b must be float64")
    if inner.dtype != _capi.F32:
        raise ValueError("multigrid.cg_solve_mixed: the inner hierarchy must be float32")
    if x.box != outer.like.box or b.box != outer.like.box:
        raise ValueError("multigrid.cg_solve_mixed: x and b must have the box of the outer level")
    if first.like.box != outer.like.box or (first.lo, first.hi) != (outer.lo, outer.hi):
        raise ValueError("multigrid.cg_solve_mixed: level 0 of the inner hierarchy must have the box and the Omega of the outer level")
    if len(inner) < 2:
        raise ValueError("multigrid.cg_solve_mixed: at least two inner levels")
    if not inner.symmetric:
        raise ValueError(_NOT_SYMMETRIC.format("cg_solve_mixed"))
    if first.lines:
        raise ValueError("multigrid.cg_solve_mixed: line stages on level 0 are not supported (levels >= 1 may have them)")
    for name in ("x", "b"):
        held = getattr(inner, name)
        if held[0] is None:
            held[0] = DeviceField.empty_like(first.like)
        elif held[0].box != first.like.box or held[0].dtype != _capi.F32:
            raise ValueError(f"multigrid.cg_solve_mixed: inner.{name}[0] must be a float32 field of level 0's box")
    if work is None:
        work = [DeviceField.empty_like(x) for _ in range(3)]
    work = list(work)
    if len(work) == 2:
        work.append(DeviceField.empty_like(x))
    if len(work) != 3 or any(f.box != x.box or f.dtype != _capi.F64 for f in work):
        raise ValueError("multigrid.cg_solve_mixed: work is two or three float64 fields like x (r, p[, q])")
    fn_dot = _apply.resolve_dot("multigrid.cg_solve_mixed", outer.entry, dot)
    arr, keep = inner._structs(inner.x[0], inner.b[0])
    out = (_capi.MgLevel * 1)()
    _fill_level(out[0], outer, x, b, work[2], keep)
    st = current_stream_ptr() if stream is None else stream
    tr = _apply.trace_buffer(3, max_iters, x.tensor, torch.float64) if trace else None
    warr = (C.c_void_p * 2)(work[0].ptr, work[1].ptr)
    done, rr0, last = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    head = (out, _capi.F64, fn_dot, arr, inner._line_structs() if inner.has_lines else None)
    rest = (len(inner), _capi.F32, sweeps, coarse_sweeps, warr, max_iters, check_every, tol2, tr.data_ptr() if trace else None, st,
            C.byref(cfg) if cfg is not None else None, C.byref(done), C.byref(rr0), C.byref(last))
    if inner.has_linear_restrict:
        _capi.check(lib.neptune_hip_mgcg_solve_mixed_transfer(*head, inner._transfer_structs(), *rest), "neptune_hip_mgcg_solve_mixed_transfer")
    else:
        _capi.check(lib.neptune_hip_mgcg_solve_mixed(*head, *rest), "neptune_hip_mgcg_solve_mixed")
    del keep
    if trace:
        return done.value, rr0.value, last.value, tr.cpu().numpy()[:3 * done.value].reshape(-1, 3).astype(np.float64, copy=False)
    return done.value, rr0.value, last.value


def smooth_dot_wide(level: Level, q: DeviceField, b: DeviceField, x: DeviceField, dot_out=None, stream: Optional[int] = None):
    """smooth(level, q, b, x) on float32 fields and the sum over Omega of b * x_new in float64, each term exact, out of the
    same launch (neptune_hip_mg_smooth_dot_wide).  dot_out: a one-element float64 device tensor to receive the sum
    (asynchronous; -> None), or None: blocking, -> the sum"""
    import torch
    if level.minv is None:
        raise ValueError("multigrid.smooth_dot_wide: the level has no minv")
    if x.dtype != _capi.F32:
        raise ValueError("multigrid.smooth_dot_wide: float32 fields only (the sum is float64)")
    st = current_stream_ptr() if stream is None else stream
    dst = dot_out if dot_out is not None else torch.zeros(1, dtype=torch.float64, device=x.tensor.device)
    _capi.check(_capi.load().neptune_hip_mg_smooth_dot_wide(_capi.F32, _capi.F64, C.byref(level.geom), q.ptr, b.ptr, level.minv.ptr,
                                                            x.ptr, dst.data_ptr(), st), "neptune_hip_mg_smooth_dot_wide")
    if dot_out is not None:
        return None
    return float(dst.item())


def coarsened_axes(fine: Level, coarse: Level) -> tuple:
    """the dimensions coarsened between two levels, as the library reads the pair (neptune_hip_mg_coarsened_axes; the others
    are kept); _capi.NeptuneHipError where the transfers would refuse the pair"""
    mask = C.c_int(0)
    _capi.check(_capi.load().neptune_hip_mg_coarsened_axes(C.byref(fine.geom), C.byref(coarse.geom), C.byref(mask)),
                "neptune_hip_mg_coarsened_axes")
    return tuple(d for d in range(fine.like.rank) if mask.value >> d & 1)


def halved_axes(fine: Level, coarse: Level) -> tuple:
    """the dimensions halved between two levels, as the library reads the pair (neptune_hip_mg_halved_axes): () for a
    vertex-centred pair; _capi.NeptuneHipError where the transfers would refuse the pair"""
    mask = C.c_int(0)
    _capi.check(_capi.load().neptune_hip_mg_halved_axes(C.byref(fine.geom), C.byref(coarse.geom), C.byref(mask)),
                "neptune_hip_mg_halved_axes")
    return tuple(d for d in range(fine.like.rank) if mask.value >> d & 1)


def smooth_dot(level: Level, q: DeviceField, b: DeviceField, x: DeviceField, dot_out=None, stream: Optional[int] = None):
    """smooth(level, q, b, x) and sum over Omega of b * x_new out of the same launch (neptune_hip_mg_smooth_dot).  dot_out: a
    one-element device tensor of x's element type to receive the sum (asynchronous; -> None), or None: blocking, -> the sum"""
    import torch
    if level.minv is None:
        raise ValueError("multigrid.smooth_dot: the level has no minv")
    st = current_stream_ptr() if stream is None else stream
    dst = dot_out if dot_out is not None else torch.zeros(1, dtype=x.tensor.dtype, device=x.tensor.device)
    _capi.check(_capi.load().neptune_hip_mg_smooth_dot(x.dtype, C.byref(level.geom), q.ptr, b.ptr, level.minv.ptr, x.ptr,
                                                       dst.data_ptr(), st), "neptune_hip_mg_smooth_dot")
    if dot_out is not None:
        return None
    return float(dst.item())


def smooth(level: Level, q: DeviceField, b: DeviceField, x: DeviceField, stream: Optional[int] = None) -> None:
    """one smoothing update on `level` from q = A(x): x = x + minv * (b - q) on Omega (neptune_hip_mg_smooth); asynchronous"""
    if level.minv is None:
        raise ValueError("multigrid.smooth: the level has no minv")
    st = current_stream_ptr() if stream is None else stream
    _capi.check(_capi.load().neptune_hip_mg_smooth(x.dtype, C.byref(level.geom), q.ptr, b.ptr, level.minv.ptr, x.ptr, st),
                "neptune_hip_mg_smooth")


def line_smooth(level: Level, stage: LineStage, q: DeviceField, b: DeviceField, x: DeviceField, stream: Optional[int] = None) -> None:
    """one line stage on `level` from q = A(x): the tridiagonal solves along stage.axis on Omega and x = x + e
    (neptune_hip_mg_line_smooth); q on Omega is overwritten; asynchronous"""
    st = current_stream_ptr() if stream is None else stream
    _capi.check(_capi.load().neptune_hip_mg_line_smooth(x.dtype, C.byref(level.geom), int(stage.axis), q.ptr, b.ptr, stage.lo.ptr,
                                                        stage.inv.ptr, stage.up.ptr, x.ptr, st), "neptune_hip_mg_line_smooth")


def line_first(level: Level, stage: LineStage, b: DeviceField, x: DeviceField, stream: Optional[int] = None) -> None:
    """the apply-free line stage on `level`: the values of line_smooth on q = +0, x = +0, from b alone
    (neptune_hip_mg_line_first); x on Omega is overwritten without being read; asynchronous"""
    st = current_stream_ptr() if stream is None else stream
    _capi.check(_capi.load().neptune_hip_mg_line_first(x.dtype, C.byref(level.geom), int(stage.axis), b.ptr, stage.lo.ptr, stage.inv.ptr,
                                                       stage.up.ptr, x.ptr, st), "neptune_hip_mg_line_first")


def line_smooth_dot(level: Level, stage: LineStage, q: DeviceField, b: DeviceField, x: DeviceField, dot_out=None,
                    stream: Optional[int] = None):
    """line_smooth(level, stage, q, b, x) and sum over Omega of b * x_new out of the same launch
    (neptune_hip_mg_line_smooth_dot).  dot_out: a one-element device tensor of x's element type to receive the sum
    (asynchronous; -> None), or None: blocking, -> the sum"""
    import torch
    st = current_stream_ptr() if stream is None else stream
    dst = dot_out if dot_out is not None else torch.zeros(1, dtype=x.tensor.dtype, device=x.tensor.device)
    _capi.check(_capi.load().neptune_hip_mg_line_smooth_dot(x.dtype, C.byref(level.geom), int(stage.axis), q.ptr, b.ptr, stage.lo.ptr,
                                                            stage.inv.ptr, stage.up.ptr, x.ptr, dst.data_ptr(), st),
                "neptune_hip_mg_line_smooth_dot")
    if dot_out is not None:
        return None
    return float(dst.item())


def restrict(fine: Level, coarse: Level, b_fine: DeviceField, q_fine: DeviceField, b_coarse: DeviceField, x_coarse: DeviceField,
             stream: Optional[int] = None) -> None:
    """b_coarse = fine.rscale * R(b_fine - q_fine) and x_coarse = +0 on the coarse Omega (neptune_hip_mg_restrict); R runs
    along the dimensions the pair coarsens (coarsened_axes) and is the identity along the kept ones; asynchronous.
    fine.restrict = "linear": the transposed linear restriction of a cell-centred pair by fine.faces
    (neptune_hip_mg_restrict_linear)"""
    st = current_stream_ptr() if stream is None else stream
    if fine.restrict_linear:
        _capi.check(_capi.load().neptune_hip_mg_restrict_linear(b_fine.dtype, C.byref(fine.geom), C.byref(coarse.geom),
                                                                C.byref(fine.transfer_struct()), b_fine.ptr, q_fine.ptr, fine.rscale,
                                                                b_coarse.ptr, x_coarse.ptr, st), "neptune_hip_mg_restrict_linear")
        return
    _capi.check(_capi.load().neptune_hip_mg_restrict(b_fine.dtype, C.byref(fine.geom), C.byref(coarse.geom), b_fine.ptr, q_fine.ptr,
                                                     fine.rscale, b_coarse.ptr, x_coarse.ptr, st), "neptune_hip_mg_restrict")


def prolong_add(fine: Level, coarse: Level, x_coarse: DeviceField, x_fine: DeviceField, stream: Optional[int] = None) -> None:
    """x_fine = x_fine + P(x_coarse) on the fine Omega (neptune_hip_mg_prolong_add); P interpolates along the dimensions
    the pair coarsens and is the identity along the kept ones; asynchronous.  fine.prolong = "linear": the linear
    prolongation of a cell-centred pair by fine.faces (neptune_hip_mg_prolong_add_linear)"""
    st = current_stream_ptr() if stream is None else stream
    if fine.linear:
        _capi.check(_capi.load().neptune_hip_mg_prolong_add_linear(x_fine.dtype, C.byref(fine.geom), C.byref(coarse.geom),
                                                                   C.byref(fine.prolong_struct()), x_coarse.ptr, x_fine.ptr, st),
                    "neptune_hip_mg_prolong_add_linear")
        return
    _capi.check(_capi.load().neptune_hip_mg_prolong_add(x_fine.dtype, C.byref(fine.geom), C.byref(coarse.geom), x_coarse.ptr,
                                                        x_fine.ptr, st), "neptune_hip_mg_prolong_add")
