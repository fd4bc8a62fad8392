"""Data, exact references and error bounds for neptune_ir.reduce {kind = "sum"} (no GPU needed).

Exact data.  Integer-valued cells (optionally times one power of two) with sum|x_i| <= 2^p, p = 53 (f64) or 24 (f32):
every partial sum of every subset is then an integer multiple of the scale of magnitude <= 2^p, so it is representable
and ANY summation order -- the oracle's serial loop, the device's fixed tree -- returns the exact sum bit for bit.
exact_sum() computes that sum with integer arithmetic and rounds it once, after checking that the rounding is exact.

Tree height.  For general data Higham's bound |s_hat - s| <= gamma_h * sum|x_i| holds with h the height of the
summation tree actually used.  tree_height() computes h from the launch arithmetic of the host code and the loop
structure of the kernels; gamma() is next to it.

Sentinels.  The masks of the cells a correct kernel never reads; the GPU tests fill them with NaN, so an over-read or a
leaked discarded value turns the result into NaN."""
import math
from fractions import Fraction

import numpy as np

P_BITS = {np.dtype(np.float64): 53, np.dtype(np.float32): 24}
VK = {np.dtype(np.float64): 2, np.dtype(np.float32): 4}   # cells per 16-byte vector
K_REDUCE_BLOCKS = 2048                                    # kReduceBlocks, csrc/kernels/util_kernels.hpp
K_REDUCE_APPLY_ITER = 8                                   # kReduceApplyIter, csrc/kernels/reduce_apply.hpp
BLOCK = 256                                               # every reduce kernel runs 256 lanes
SHUFFLE_LEVELS = 6                                        # block_sum: __shfl_down by 32, 16, ..., 1 (kWave = 64)
LDS_CHAIN = 4                                             # block_sum: thread 0 adds the 4 wave sums, r = 0 + ...


def _p(dtype):
    return P_BITS[np.dtype(dtype)]


def _cdiv(a, b):
    return -(-a // b)


# ---- exact data ---------------------------------------------------------------------------------------------------
def exact_field(shape, dtype, seed, scale_exp=0, bound_bits=None, sparse=None, max_abs=None):
    """integer-valued cells in [-M, M] times 2**scale_exp, sum|x| <= 2^bound_bits (default p of the dtype).

    M defaults to the largest value the bound allows for the whole array, capped at 2^30: f64 cells of up to 30
    significant bits, or partial sums of more than 24 (2^20 over 10^5 cells needs 37), make an accumulator narrower
    than the element type round.  sparse: fraction of non-zero cells.  scale_exp = -1074 (f64) / -149 (f32) gives all-subnormal cells whose exact sum is representable."""
    dtype = np.dtype(dtype)
    bits = _p(dtype) if bound_bits is None else bound_bits
    assert bits <= _p(dtype)
    shape = tuple(int(n) for n in shape)
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    if max_abs is None:
        dens = 1.0 if sparse is None else sparse
        max_abs = max(1, min(1 << 30, int((1 << bits) // max(1, int(math.ceil(n * dens))))))
    v = rng.integers(-max_abs, max_abs + 1, size=n, dtype=np.int64)
    if sparse is not None:
        v[rng.random(n) >= sparse] = 0
    total = int(np.abs(v).sum())
    while total > (1 << bits):                     # only the rare tail of a dense draw: thin it out
        nz = np.flatnonzero(v)
        v[nz[: len(nz) // 8 + 1]] = 0
        total = int(np.abs(v).sum())
    x = np.ldexp(v.astype(np.float64), scale_exp).astype(dtype)
    assert np.array_equal(np.ldexp(x.astype(np.float64), -scale_exp), v.astype(np.float64)), "scaled cells not exact"
    assert abs_sum_exact(x) <= Fraction(2) ** (bits + scale_exp)
    return x.reshape(shape)


def box_slices(box, ndim):
    """numpy slices of box = (lo, hi) in array indices (None: everything); a backwards axis is empty"""
    if box is None:
        return (slice(None),) * ndim
    lo, hi = box
    return tuple(slice(int(l), max(int(l), int(h))) for l, h in zip(lo, hi))


def _exact_fraction(x):
    """sum of the cells of x as a Fraction (x finite)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)   # f32 -> f64 is exact
    x = x[x != 0]
    if x.size == 0:
        return Fraction(0)
    assert np.isfinite(x).all(), "exact_sum of non-finite data"
    m, ex = np.frexp(x)
    k = np.ldexp(m, 53).astype(np.int64)                 # x = k * 2^(ex - 53), k an integer
    tz = np.zeros(k.shape, np.int64)
    kk = np.abs(k)
    for s in (32, 16, 8, 4, 2, 1):                       # trailing zero bits of k
        sel = (kk & ((1 << s) - 1)) == 0
        tz[sel] += s
        kk[sel] >>= s
    e = int((ex - 53 + tz).min())                        # every cell is an integer multiple of 2^e
    q = np.ldexp(x, -e)                                  # exact: an exponent shift
    if float(np.abs(q).max()) * x.size < 2.0 ** 62:
        s = int(q.astype(np.int64).sum())
    else:
        s = sum(int(v) for v in q)
    return Fraction(s) * (Fraction(2) ** e)


def abs_sum_exact(x):
    return _exact_fraction(np.abs(np.asarray(x)))


def exact_sum(x, box=None):
    """the exact sum of x[box] (box = (lo, hi) in array indices; an empty or backwards box sums to 0), rounded once to
    x's dtype -- and that rounding must be exact"""
    x = np.asarray(x)
    dt = x.dtype.type
    s = _exact_fraction(x[box_slices(box, x.ndim)])
    r = dt(float(s))
    assert Fraction(float(r)) == s, f"exact sum {s} is not representable in {x.dtype}"
    return dt(0) if s == 0 else r   # +0.0 for an empty box or an all-zero (incl. all -0.0) box


# ---- sentinel placement -------------------------------------------------------------------------------------------
def plain_sentinel_mask(shape, box):
    """True at every buffer cell a reduce over box (array indices) must not read"""
    m = np.ones(shape, bool)
    m[box_slices(box, len(shape))] = False
    return m


def _box_and(a, b):
    return tuple(max(x, y) for x, y in zip(a[0], b[0])), tuple(min(x, y) for x, y in zip(a[1], b[1]))


def fused_sentinel_masks(result_box, bounds, reduce_box, input_boxes, footprints):
    """reduce(apply): one mask per input, True at the cells a correct kernel never uses.  All boxes are logical
    (lb, ub) pairs; footprints[k] is the list of offsets input k is read at.  Used: (R & B) + footprint_k, and for input
    0 also the copy-through cells, i.e. all of R (input 0 shares the result's box)."""
    rb = _box_and(reduce_box, bounds)
    masks = []
    for k, (ilb, iub) in enumerate(input_boxes):
        shape = tuple(u - l for l, u in zip(ilb, iub))
        m = np.ones(shape, bool)
        if all(h > l for l, h in zip(*rb)):
            for off in footprints[k]:
                lo = [l + o - b for l, o, b in zip(rb[0], off, ilb)]
                hi = [h + o - b for h, o, b in zip(rb[1], off, ilb)]
                assert all(0 <= a and c <= n for a, c, n in zip(lo, hi, shape)), "footprint leaves the input box"
                m[tuple(slice(a, c) for a, c in zip(lo, hi))] = False
        if k == 0 and all(h > l for l, h in zip(*reduce_box)):
            m[tuple(slice(l - b, h - b) for l, h, b in zip(reduce_box[0], reduce_box[1], result_box[0]))] = False
        masks.append(m)
    return masks


# ---- launch geometry and tree height ------------------------------------------------------------------------------
def plain_path(shape, box, aligned=True):
    """the first-pass kernel neptune_hip_reduce picks (reduce_plan in csrc/runtime/neptune_hip_rt.hip, `whole`): the flat
    kernel for the whole buffer at a 16-byte-aligned base, the box kernel otherwise"""
    lo, hi = box if box is not None else ((0,) * len(shape), tuple(shape))
    whole = all(l == 0 and h == n for l, h, n in zip(lo, hi, shape)) and aligned
    return "flat" if whole else "box"


def fused_path(dtype, pointwise, result_shape, reduce_lo, reduce_hi, inputs_share_result_box):
    """the first-pass kernel a fused reduce(apply) picks (plan_reduce_apply in csrc/kernels/reduce_launch.hpp, `vec`): the
    vector kernel for a pointwise body (run_apply_reduce_op: FP::MARCH_OK && FP::HALO_MASK == 0) when eK, the reduced box's first K index and the row
    length are multiples of VK and every input is 16-byte aligned and has the result's box (sh == 0, m == n); all
    coordinates here are result-physical, K the last axis"""
    v = VK[np.dtype(dtype)]
    ek = reduce_hi[-1] - reduce_lo[-1]
    vec = pointwise and ek % v == 0 and reduce_lo[-1] % v == 0 and result_shape[-1] % v == 0 and inputs_share_result_box
    return "fused_vec" if vec else "fused_scalar"


def launch_blocks(path, dtype, ext):
    """first-pass grid size, as the host computes it.  ext: the reduced box's extents (flat: (count,))"""
    v = VK[np.dtype(dtype)]
    total = int(np.prod(ext))
    rows, last = total // max(ext[-1], 1), ext[-1]
    if path == "flat":          # reduce_plan: min(ceil(total / 256), kReduceBlocks)
        return min(_cdiv(total, 256), K_REDUCE_BLOCKS)
    if path == "box":           # reduce_plan, !whole: trips of 4 chunks of 256 * VK cells
        trips = _cdiv(rows * _cdiv(last, 256 * v), 4)
        return min(max(trips, 1), K_REDUCE_BLOCKS)
    cells, it = (256 * v, K_REDUCE_APPLY_ITER // 2) if path == "fused_vec" else (256, K_REDUCE_APPLY_ITER)
    trips = _cdiv(rows * _cdiv(last, cells), it)     # plan_reduce_apply
    return min(trips, K_REDUCE_BLOCKS)


# The host and kernel lines the functions above restate, verbatim (paths relative to neptune-pde-solver_amd/csrc).
# tests/test_reduce_cases.py checks that each is still there, so a change to the kernel choice, the grid or the
# loop structure fails a CPU test until this mirror is brought up to date with it.  A host rule has ONE home: each line
# of MIRRORED_HOST must occur in no other file under csrc and only once in its own, so a second copy of a launch rule,
# which could drift from the mirrored one with every test green, fails that test too.
MIRRORED_HOST = [
    # the plain reduce: reduce_plan (the kernel choice `whole`, the grid) and reduce_launch
    ("runtime/neptune_hip_rt.hip", "whole = whole && off[d] == 0 && ext[d] == shp[d] && ((uintptr_t)src % 16 == 0);"),
    ("runtime/neptune_hip_rt.hip", "int blocks = (int)((total + 255) / 256 < kReduceBlocks ? (total + 255) / 256 : kReduceBlocks);"),
    ("runtime/neptune_hip_rt.hip", "const int64_t cells = 256 * (dtype == NEPTUNE_HIP_F64 ? 2 : 4);"),
    ("runtime/neptune_hip_rt.hip", "const int64_t trips = ((total / (last ? last : 1)) * ((last + cells - 1) / cells) + 3) / 4;"),
    ("runtime/neptune_hip_rt.hip", "blocks = (int)(trips < kReduceBlocks ? (trips < 1 ? 1 : trips) : kReduceBlocks);"),
    # reduce(apply): plan_reduce_apply (the kernel choice `vec`, the grid), launch_reduce_apply and launch_reduce_root;
    # run_apply_reduce_op (lowered_runtime.hpp) passes `pointwise`
    ("kernels/reduce_launch.hpp", "bool vec = pointwise && eK % VK == 0 && P.rlb[2] % VK == 0 && P.n[2] % VK == 0;"),
    ("kernels/reduce_launch.hpp", "vec = vec && ((uintptr_t)ptrs[k] % 16 == 0);"),
    ("kernels/reduce_launch.hpp", "for (int ax = 0; ax < 3; ++ax) vec = vec && P.sh[k][ax] == 0 && P.m[k][ax] == P.n[ax];"),
    ("kernels/reduce_launch.hpp",
     "const int cells_per_chunk = 256 * (vec ? VK : 1), iter = vec ? kReduceApplyIter / 2 : kReduceApplyIter;"),
    ("kernels/reduce_launch.hpp",
     "const int64_t trips = ((P.rub[0] - P.rlb[0]) * (P.rub[1] - P.rlb[1]) * nchunk + iter - 1) / iter;"),
    ("kernels/reduce_launch.hpp", "const int blocks = (int)(trips < kReduceBlocks ? trips : kReduceBlocks);"),
    ("kernels/reduce_launch.hpp", "hipLaunchKernelGGL((neptune_reduce_final<T, FOp>), dim3(1), dim3(256)"),
    ("kernels/reduce_launch.hpp", "hipLaunchKernelGGL((neptune_reduce_apply<Body, T, RANK, NIN, POp>), dim3(pl.blocks), dim3(256)"),
    ("runtime/lowered_runtime.hpp", "constexpr bool kPointwise = FP::MARCH_OK && FP::HALO_MASK == 0u;"),
]
MIRRORED_KERNEL = [
    ("kernels/util_kernels.hpp", "constexpr int kReduceBlocks = 2048;"),
    ("kernels/util_kernels.hpp", "for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o);"),
    ("kernels/util_kernels.hpp", "for (int i = 0; i < nw; ++i) r += lds[i];"),
    ("kernels/util_kernels.hpp", "const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;"),
    ("kernels/util_kernels.hpp", "for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {"),
    ("kernels/util_kernels.hpp", "for (int64_t i = nvec * VK; i < count; ++i) acc += src[i];"),
    ("kernels/util_kernels.hpp", "constexpr int VK = 16 / sizeof(T), ITER = 4;"),
    ("kernels/util_kernels.hpp", "for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];"),
    ("kernels/apply_common.hpp", "constexpr int kWave = 64;"),
    ("kernels/reduce_apply.hpp", "constexpr int kReduceApplyIter = 8;"),
    ("kernels/reduce_apply.hpp", "for (int it = 0; it < kReduceApplyIter; ++it) acc += v[it];"),
    ("kernels/reduce_apply.hpp", "constexpr int ITER = kReduceApplyIter / 2;"),
]
MIRRORED = MIRRORED_HOST + MIRRORED_KERNEL


def _final_height(blocks):
    # neptune_reduce_final (util_kernels.hpp): lane t adds partials t, t + 256, ... to 0, then block_sum
    # (6 shuffle levels, thread 0 adds the 4 wave sums to 0)
    return _cdiv(blocks, BLOCK) + SHUFFLE_LEVELS + LDS_CHAIN


def tree_height(path, dtype, ext):
    """an upper bound on the number of additions on any path from a cell to the result, from the loop structure of the
    kernels (util_kernels.hpp, reduce_apply.hpp) and the grid of launch_blocks().  It counts the first addition of
    every chain to its zero accumulator, which is exact: these spare levels also cover the rounding of a correctly
    rounded reference such as math.fsum.  path: flat | box | fused_scalar | fused_vec."""
    v = VK[np.dtype(dtype)]
    ext = tuple(int(e) for e in ext)
    total = int(np.prod(ext))
    if total == 0:
        return 0
    blocks = launch_blocks(path, dtype, ext)
    rows, last = total // ext[-1], ext[-1]
    if path == "flat":
        # neptune_reduce_partial_flat: per = ceil(nvec / blocks) vectors per workgroup, lane-strided by 256 into VK
        # partials each, those VK partials added in order, then (last workgroup, lane 0) the count % VK tail cells,
        # counted as VK - 1 whatever the tail so that h stays monotone in n
        nvec = total // v
        per = _cdiv(nvec, blocks)
        h = _cdiv(per, BLOCK) + v + (v - 1)
    elif path == "box":
        # neptune_reduce_partial_box: per = ceil(chunks / blocks), trips of ITER = 4 chunks, each adding one cell to
        # each of VK partials; then the VK partials in order
        per = _cdiv(rows * _cdiv(last, 256 * v), blocks)
        h = 4 * _cdiv(per, 4) + v
    elif path == "fused_scalar":
        # neptune_reduce_apply: trips of ITER = 8 chunks, one cell per chunk per lane, one accumulator
        per = _cdiv(rows * _cdiv(last, 256), blocks)
        h = K_REDUCE_APPLY_ITER * _cdiv(per, K_REDUCE_APPLY_ITER)
    elif path == "fused_vec":
        # neptune_reduce_apply_vec: trips of ITER = 4 chunks, VK cells per chunk per lane, one accumulator
        it = K_REDUCE_APPLY_ITER // 2
        per = _cdiv(rows * _cdiv(last, 256 * v), blocks)
        h = it * v * _cdiv(per, it)
    else:
        raise ValueError(path)
    return h + SHUFFLE_LEVELS + LDS_CHAIN + _final_height(blocks)


def unit_roundoff(dtype):
    return 2.0 ** -_p(dtype)


def gamma(h, dtype):
    """gamma_h = h u / (1 - h u), u the unit roundoff of dtype (Higham, Accuracy and Stability, 2nd ed., 3.1 and 4.2)"""
    hu = h * unit_roundoff(dtype)
    assert hu < 1
    return hu / (1 - hu)


def serial_bound(n, dtype):
    """the bound the older tests use: 2 (n - 1) eps"""
    return 2.0 * max(n - 1, 0) * float(np.finfo(dtype).eps)


# ---- reduce(apply) modules ----------------------------------------------------------------------------------------
def _bnd(box):
    return f"#neptune_ir.bounds<lb = [{', '.join(map(str, box[0]))}], ub = [{', '.join(map(str, box[1]))}]>"


def _unit(rank, axis, o):
    return tuple(o if d == axis else 0 for d in range(rank))


BODIES = ("sum", "dot", "stencil", "div")


def body_footprints(body, rank, nin):
    """offsets at which the body reads each input"""
    z = (0,) * rank
    if body in ("sum", "dot", "div"):
        return [[z] for _ in range(nin)]
    assert body == "stencil"
    fp = [[z, _unit(rank, rank - 1, -1), _unit(rank, 0, 1)], [z, _unit(rank, rank - 1, 1)], [z, _unit(rank, 0, -1)]]
    return fp[:nin]


def fused_module(elem, result_box, bounds, reduce_box, input_boxes, body):
    """-> (text, footprints).  @red(ins...) -> elem: reduce(apply(ins){body}) over reduce_box, the apply result used
    once, which the lowering fuses into one reduce kernel.  @vals(out, ins...): the same apply stored whole into out,
    for the oracle's per-cell values.  Input 0 has the result's box; the other inputs may have boxes of their own.

    body: sum (x0 + x1 + ...), dot (x0 * x1 [+ x2]; x0 * x0 for one input), div (x0 / x1), all pointwise; stencil
    (input 0 at 0, -1 along the last axis and +1 along the first, input 1 at 0 and +1 along the last, input 2 at 0 and
    -1 along the first, added with signs)."""
    rank = len(result_box[0])
    nin = len(input_boxes)
    assert tuple(map(tuple, input_boxes[0])) == tuple(map(tuple, result_box))
    mr = "memref<" + "x".join("?" * rank) + "x" + elem + ">"
    boxes = [tuple(map(tuple, result_box))] + [tuple(map(tuple, b)) for b in input_boxes]
    uniq = list(dict.fromkeys(boxes))
    ty = {b: i for i, b in enumerate(uniq)}
    defs = []
    for b, i in ty.items():
        defs.append(f"!t{i} = !neptune_ir.temp<element = {elem}, bounds = {_bnd(b)}, location = #l>")
        defs.append(f"!f{i} = !neptune_ir.field<element = {elem}, bounds = {_bnd(b)}, location = #l>")
    tin = [ty[tuple(map(tuple, b))] for b in input_boxes]
    tres = ty[boxes[0]]
    fps = body_footprints(body, rank, nin)
    lines, names = [], {}
    for k in range(nin):
        for j, off in enumerate(fps[k]):
            nm = f"%x{k}_{j}"
            names[(k, off)] = nm
            lines.append(f"        {nm} = neptune_ir.access %p{k}[{', '.join(map(str, off))}] : !t{tin[k]} -> {elem}")
    z = (0,) * rank
    c = [names[(k, z)] for k in range(nin)]
    if body == "sum":
        acc = c[0]
        for k in range(1, nin):
            lines.append(f"        %s{k} = arith.addf {acc}, {c[k]} : {elem}")
            acc = f"%s{k}"
    elif body == "dot":
        lines.append(f"        %m = arith.mulf {c[0]}, {c[1] if nin > 1 else c[0]} : {elem}")
        acc = "%m"
        if nin > 2:
            lines.append(f"        %m2 = arith.addf %m, {c[2]} : {elem}")
            acc = "%m2"
    elif body == "div":
        assert nin == 2
        lines.append(f"        %q = arith.divf {c[0]}, {c[1]} : {elem}")
        acc = "%q"
    else:
        terms = [(k, off, -1 if (j == 1 and k == 0) or (j == 1 and k == 2) else 1)
                 for k in range(nin) for j, off in enumerate(fps[k])]
        acc = names[(terms[0][0], terms[0][1])]
        for t, (k, off, sgn) in enumerate(terms[1:]):
            lines.append(f"        %t{t} = arith.{'addf' if sgn > 0 else 'subf'} {acc}, {names[(k, off)]} : {elem}")
            acc = f"%t{t}"
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    bargs = ", ".join(f"%p{k}: !t{tin[k]}" for k in range(nin))
    targs = ", ".join(f"!t{tin[k]}" for k in range(nin))
    apply = (f"    %w = neptune_ir.apply({', '.join(f'%u{k}' for k in range(nin))}) attributes {{bounds = {_bnd(bounds)}}} "
             f": ({targs}) -> !t{tres} {{\n      ^bb0({idx}, {bargs}):\n" + "\n".join(lines)
             + f"\n        neptune_ir.yield {acc} : {elem}\n    }}\n")
    loads = "".join(f"    %g{k} = neptune_ir.wrap %a{k} : {mr} -> !f{tin[k]}\n"
                    f"    %u{k} = neptune_ir.load %g{k} : !f{tin[k]} -> !t{tin[k]}\n" for k in range(nin))
    params = ", ".join(f"%a{k}: {mr}" for k in range(nin))
    text = f"""
#l = #neptune_ir.location<"cell">
{chr(10).join(defs)}
module {{
  func.func @red({params}) -> {elem} {{
{loads}{apply}    %s = neptune_ir.reduce %w in {_bnd(reduce_box)} {{kind = "sum"}} : !t{tres} -> {elem}
    func.return %s : {elem}
  }}
  func.func @vals(%out: {mr}, {params}) -> {mr} {{
    %fo = neptune_ir.wrap %out : {mr} -> !f{tres}
{loads}{apply}    neptune_ir.store %w to %fo : !t{tres} to !f{tres}
    %r = neptune_ir.unwrap %fo : !f{tres} -> {mr}
    func.return %r : {mr}
  }}
}}
"""
    return text, fps


def plain_module(elem, box, reduce_box=None):
    """@red(a) -> elem: neptune_ir.reduce of a loaded field of any rank 1..6, over reduce_box or the whole field"""
    rank = len(box[0])
    mr = "memref<" + "x".join("?" * rank) + "x" + elem + ">"
    where = "" if reduce_box is None else f" in {_bnd(reduce_box)}"
    return f"""
#l = #neptune_ir.location<"cell">
!t = !neptune_ir.temp<element = {elem}, bounds = {_bnd(box)}, location = #l>
!f = !neptune_ir.field<element = {elem}, bounds = {_bnd(box)}, location = #l>
module {{
  func.func @red(%a: {mr}) -> {elem} {{
    %f = neptune_ir.wrap %a : {mr} -> !f
    %u = neptune_ir.load %f : !f -> !t
    %s = neptune_ir.reduce %u{where} {{kind = "sum"}} : !t -> {elem}
    func.return %s : {elem}
  }}
}}
"""


# ---- the general-data cases of the GPU tests (tests/test_reduce_exact_gpu.py), one list per first-pass kernel -----
# plain: (buffer shape, reduced box in array indices or None); fused: (result shape, reduced box), both rank 1..3
GAMMA_PLAIN = {
    "flat": [((1_000_003,), None), ((64, 96, 128), None), ((600_001,), None)],
    "box": [((37, 129), ((5, 0), (30, 100))), ((20, 33, 65), ((2, 5, 7), (19, 30, 60))), ((300, 2051), ((1, 1), (299, 2050)))],
}
GAMMA_FUSED = {
    "fused_scalar": [((9, 7, 300), ((0, 1, 1), (9, 5, 298))), ((70000,), ((0,), (70000,))), ((600, 1000), ((0, 1), (599, 999)))],
    "fused_vec": [((33, 4096), ((0, 0), (32, 4096))), ((7, 9, 1100), ((0, 0, 0), (6, 9, 1100))), ((1_000_000,), ((0,), (1_000_000,)))],
}


def box_ext(shape, box):
    if box is None:
        return tuple(shape)
    return tuple(max(0, h - l) for l, h in zip(*box))
