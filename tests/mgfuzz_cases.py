"""Composed multigrid hierarchies, fuzzed: a seeded generator of hierarchies that mix what the features' case
modules test one at a time, run on mg_restatement.  A level's operator is mg_restatement.OmegaOperator: the oracle's A on
Omega and +0 on every other cell.

decode(seed) draws a case from a fixed pool of module templates (TEMPLATES): a template fixes
rank, element type, the boxes (unequal rims of 1..3 cells), the modules' bounds and, per pair, the dimensions transferred --
so also the weights per level, by the plan rule (w on a transferred dimension, 4 w on a kept one).  Everything else is drawn
and costs no compile: how many of the template's levels are used, Omega inside the bounds (a launch region), and with it the
GRID KIND of every pair -- bounds of 264 -> 132 -> 66 -> 33 hold 264 -> 132 -> 66 -> 33 (halved), 263 -> 131 -> 65 -> 32
(coarsened), 262 -> 131 -> 65 and 261 -> 130 -> 65 (the kind switches) --, the line stages per level, the schedule, the launch
path and the allocation offset.  build(case) makes the restatement's levels and the problem's fields."""
import sys

import numpy as np

import helpers
import mg_restatement as rst
import mgcg_cases as mg
import mgcgmixed_cases as mx
import mglines_cases as lc
import monitor_cases as mc
from mg_restatement import Halved

D, S = np.float64, np.float32
DAMP = 0.8

# name: (element type of the hierarchy, [the module's bounds extents per level], [the dimensions transferred per pair],
#        whether an f64 outer operator of level 0 exists (mixed precision))
# Transferred extents double from level to level (or double plus one), kept ones stay: Omega, drawn inside the bounds,
# decides the grid kind of a pair.  The contiguous chains are the ones that cross the 256-cell chunk with a short tail
# (264 / 263 / 262 / 261), the short ones give rows below a wave and levels of one or two cells.
TEMPLATES = {
    "r1_long":   (D, [(264,), (132,), (66,), (33,)], [(0,)] * 3, False),
    "r1_short":  (S, [(16,), (8,), (4,), (2,)], [(0,)] * 3, False),
    "r2_odd":    (D, [(15, 263), (7, 131), (3, 65), (1, 32)], [(0, 1)] * 3, False),
    "r2_semi":   (S, [(14, 264), (14, 132), (7, 66), (7, 33)], [(1,), (0, 1), (1,)], True),
    "r2_lines":  (D, [(70, 16), (70, 8), (70, 4)], [(1,), (1,)], False),
    "r2_even":   (S, [(16, 264), (8, 132), (4, 66)], [(0, 1)] * 2, True),
    "r3_even":   (D, [(8, 16, 264), (4, 8, 132), (2, 4, 66)], [(0, 1, 2)] * 2, False),
    "r3_odd":    (S, [(7, 15, 263), (3, 7, 131), (1, 3, 65)], [(0, 1, 2)] * 2, True),
    "r3_2":      (D, [(3, 7, 264), (3, 7, 132)], [(2,)], False),
    "r3_1":      (S, [(2, 14, 70), (2, 7, 70)], [(1,)], False),
    "r3_0":      (D, [(14, 3, 33), (7, 3, 33)], [(0,)], False),
    "r3_01":     (S, [(6, 14, 15), (3, 7, 15)], [(0, 1)], False),
    "r3_02":     (D, [(6, 1, 264), (3, 1, 132)], [(0, 2)], False),
    "r3_12":     (S, [(1, 16, 32), (1, 8, 16)], [(1, 2)], False),
}
FORMS = {0: "solve", 1: "cg", 2: "cg-lines", 3: "mixed", 9: "refused"}
REFUSALS = ("mixed_kinds", "mixed_stage0", "stage_axis")


def seed_class(seed):
    """the form a seed draws: the thousands say it"""
    return FORMS[seed // 1000]


def template_levels(name):
    """-> per level (box shape, bounds (lb, ub), weights): rims of 1..3 cells, unequal, fixed per level and dimension"""
    _, extents, transferred, _ = TEMPLATES[name]
    rank = len(extents[0])
    w, out = tuple(1.0 for _ in range(rank)), []
    for l, B in enumerate(extents):
        lo = [1 + (l + d) % 3 for d in range(rank)]
        hi = [1 + (l + 2 * d + 1) % 3 for d in range(rank)]
        shape = tuple(a + n + b for a, n, b in zip(lo, B, hi))
        out.append((shape, (lo, [a + n for a, n in zip(lo, B)]), w))
        if l + 1 < len(extents):
            w = tuple(v if d in transferred[l] else 4.0 * v for d, v in enumerate(w))
    return out


def module_text(name, level, dtype):
    """the operator -sum_d w_d u_dd of a template's level, unscaled: monitor_cases.star_module where all weights are equal,
    mgcg_cases.aniso_module otherwise"""
    shape, bounds, w = template_levels(name)[level]
    if len(set(w)) == 1:
        return mc.star_module(shape, dtype, bounds=bounds, centre=2.0 * len(shape) * w[0], side=-w[0])
    return mg.aniso_module(shape, w, dtype, bounds=bounds)


def case_modules(case):
    """[(module text, compiled with its dot entry)] of a case: the outer operator of a mixed case first, then the levels;
    level 0 of every template is compiled with its dot entry (the CG forms need it, solve() launches the plain entry of the
    same object)"""
    name = case["template"]
    out = [(module_text(name, 0, D), True)] if case["form"] == "mixed" or case.get("why") == "mixed_stage0" else []
    return out + [(module_text(name, l, case["dtype"]), l == 0) for l in range(case["n_levels"])]


def _native_kinds(extents, transferred):
    """the grid kind of each pair when Omega is the bounds themselves; None when the bounds do not nest"""
    kinds = []
    for l, axes in enumerate(transferred):
        ks = {"H" if extents[l][d] == 2 * extents[l + 1][d] else "C" if extents[l][d] == 2 * extents[l + 1][d] + 1 else "?" for d in axes}
        if len(ks) != 1 or "?" in ks or any(extents[l][d] != extents[l + 1][d] for d in range(len(extents[0])) if d not in axes):
            return None
        kinds.append(ks.pop())
    return kinds


def _chain(m_last, transferred, kinds):
    """Omega's extents per level from the coarsest upward: 2 m + 1 (coarsened), 2 m (halved) or m (kept)"""
    out = [tuple(m_last)]
    for axes, kind in zip(reversed(transferred), reversed(kinds)):
        out.append(tuple((2 * m + (kind == "C") if d in axes else m) for d, m in enumerate(out[-1])))
    return out[::-1]


def decode(seed):
    """the full description of a case, a dict of plain values; deterministic"""
    rng = np.random.default_rng(seed)
    form = seed_class(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    case = {"seed": seed, "form": form}
    if form == "refused":
        why = REFUSALS[seed % len(REFUSALS)]
        name = {"mixed_kinds": "r3_01", "mixed_stage0": "r2_even", "stage_axis": "r2_odd"}[why]
        dtype, extents, transferred, _ = TEMPLATES[name]
        n_levels = 2
        m = [extents[0], extents[1]]
        stages = [[], []]
        if why == "mixed_kinds":        # dimension 0 halved, 6 -> 3, and dimension 1 coarsened, 13 -> 6, in one pair
            m = [(6, 13, 15), (3, 6, 15)]
        elif why == "mixed_stage0":
            stages = [[1], [0]]
        else:
            stages = [[], [len(extents[0])]]
        kinds = ["H" if why != "stage_axis" else "C"]
        case.update(why=why)
    else:
        names = sorted(TEMPLATES)
        if form == "mixed":
            names = [n for n in names if TEMPLATES[n][3]]
        name = pick(names)
        dtype, extents, transferred, _ = TEMPLATES[name]
        n_levels = int(rng.integers(2, len(extents) + 1))
        extents, transferred = extents[:n_levels], transferred[:n_levels - 1]
        rank = len(extents[0])
        native = _native_kinds(extents, transferred)
        assert native is not None, name
        narrowed = bool(rng.integers(2))
        m, kinds = list(extents), native
        for _ in range(64 if narrowed else 0):
            ks = [pick("CH") for _ in transferred]
            last = [int(rng.integers(1, B + 1)) if B <= 4 else int(B - rng.integers(0, 3)) for B in extents[-1]]
            cand = _chain(last, transferred, ks)
            if min(last) >= 1 and all(v <= B for mm, BB in zip(cand, extents) for v, B in zip(mm, BB)) and cand != list(extents):
                m, kinds = cand, ks
                break
        k0 = {"cg": (0, 0), "mixed": (0, 0), "cg-lines": (1, 3)}.get(form)
        stages = []
        for l in range(n_levels):
            k = int(rng.integers(k0[0], k0[1] + 1)) if (k0 and l == 0) else int(pick((0, 0, 0, 1, 1, 2, 3)))
            stages.append([int(rng.integers(rank)) for _ in range(k)])
    levels = template_levels(name)
    lo = []
    for l in range(n_levels):
        lb = levels[l][1][0]
        lo.append(tuple(int(a + rng.integers(0, B - v + 1)) for a, B, v in zip(lb, TEMPLATES[name][1][l], m[l])))
    case.update(template=name, rank=len(m[0]), dtype=dtype, n_levels=n_levels, kinds=list(kinds),
                transferred=[tuple(a) for a in TEMPLATES[name][2][:n_levels - 1]], m=[tuple(v) for v in m], lo=lo,
                shapes=[levels[l][0] for l in range(n_levels)], bounds=[levels[l][1] for l in range(n_levels)],
                weights=[levels[l][2] for l in range(n_levels)], stages=stages,
                narrowed=[tuple(m[l]) != tuple(TEMPLATES[name][1][l]) for l in range(n_levels)])
    pre, post = pick(((0, 1), (0, 2), (1, 0), (2, 0), (1, 1), (1, 2), (2, 1), (2, 2)))
    case.update(pre=int(pre), post=int(post), sweeps=int(rng.integers(1, 3)), coarse_sweeps=int(rng.integers(1, 9)),
                n=int(rng.integers(1, 4)), check_every=int(rng.integers(1, 4)), graph=bool(rng.integers(2)),
                offset=int(8 * rng.integers(2)), both_paths=seed % 4 == 0)
    # one solve() case in eight works on subnormal numbers (x0 and b scaled by a power of two): a transfer that scales before
    # it adds, or a kernel that flushes, shows there and only there.  (The CG forms divide by sums of squares: not for them.)
    case["tiny"] = bool(form == "solve" and rng.integers(8) == 0)
    return case


def where_of(case, l):
    return tuple(slice(a, a + v) for a, v in zip(case["lo"][l], case["m"][l]))


def region_of(case, l):
    """the launch region that narrows the module's bounds to Omega (result-physical), None where Omega is the bounds: along a
    narrowed dimension Omega's own range, along the others the whole box"""
    if not case["narrowed"][l]:
        return None
    lb, ub = case["bounds"][l]
    cut = [v != b - a for v, a, b in zip(case["m"][l], lb, ub)]
    return ([a if c else 0 for a, c in zip(case["lo"][l], cut)],
            [a + v if c else n for a, v, c, n in zip(case["lo"][l], case["m"][l], cut, case["shapes"][l])])


def stage_factors(shape, where, weights, axis, dtype, outside=np.nan):
    """(axis, lo, inv, up): mglines_cases.factors on the tridiagonal part (-w_a, 2 sum w, -w_a) of the operator along `axis`
    over Omega, the couplings to cells outside Omega dropped; `outside` on every cell outside Omega"""
    lower, diag, upper = (np.zeros(shape, dtype) for _ in range(3))
    lower[where], diag[where], upper[where] = -weights[axis], 2.0 * sum(weights), -weights[axis]
    first, last = list(where), list(where)
    first[axis], last[axis] = where[axis].start, where[axis].stop - 1
    lower[tuple(first)] = 0.0
    upper[tuple(last)] = 0.0
    return (axis,) + lc.factors(lower, diag, upper, where, axis, DAMP, outside)


def restatement_levels(case, dtype=None):
    """the restatement's levels of a case (mg_restatement.Level with .axes, .stages, .weights): minv = DAMP / diagonal on Omega; outside
    Omega level 0's is +0 for the CG forms (they form minv_0 * r on the whole box) and NaN everywhere else, as the factor fields"""
    dtype = dtype or case["dtype"]
    dt = np.dtype(dtype).type
    name, levels = case["template"], []
    for l in range(case["n_levels"]):
        shape, where, w = case["shapes"][l], where_of(case, l), case["weights"][l]
        zero_outside = l == 0 and case["form"] in ("cg", "cg-lines", "mixed")
        minv = np.full(shape, 0.0 if zero_outside else np.nan, dtype)
        minv[where] = dt(dt(DAMP) / dt(2.0 * sum(w)))
        L = rst.Level(rst.OmegaOperator(module_text(name, l, dtype), where), shape, where, minv, dtype)
        L.weights = w
        if l + 1 < case["n_levels"]:
            L.axes = Halved(case["transferred"][l]) if case["kinds"][l] == "H" else tuple(case["transferred"][l])
        else:
            L.axes = ()
        L.stages = [stage_factors(shape, where, w, a, dtype) for a in case["stages"][l] if a < len(shape)]   # (a refused case's axis)
        levels.append(L)
    return levels


def problem_fields(case):
    """x0: hashed non-zero values outside Omega_0 and +0 inside; b: hashed, every 7th cell a -0; both read-only"""
    dtype = D if case["form"] == "mixed" or case.get("why") == "mixed_stage0" else case["dtype"]
    shape, where = case["shapes"][0], where_of(case, 0)
    x0 = helpers.hash_field(shape, dtype, seed=case["seed"] + 1)
    assert (x0 != 0).all()
    x0[where] = 0.0
    b = helpers.hash_field(shape, dtype, seed=case["seed"] + 2)
    b.reshape(-1)[case["seed"] % 7::7] = -0.0
    if case["tiny"]:            # |values| < 2^-140 (f32) or 2^-1065 (f64): all subnormal, nine or so bits each
        scale = np.dtype(dtype).type(2.0) ** (-140 if np.dtype(dtype) == S else -1065)
        x0, b = x0 * scale, b * scale
    for a in (x0, b):
        a.setflags(write=False)
    return x0, b


class Built:
    """a case ready to run: .case, .levels (the restatement's; f32 for a mixed case), .problem (what mg_restatement.setup / replay take: the
    levels, or an mgcgmixed_cases.Problem around them), .x0, .b"""


def build(case):
    B = Built()
    B.case = case
    B.levels = restatement_levels(case)
    B.problem = B.levels
    if case["form"] == "mixed":
        B.problem = mx.Problem(rst.OmegaOperator(module_text(case["template"], 0, D), B.levels[0].where), B.levels)
    B.x0, B.b = problem_fields(case)
    return B


def reference(B):
    """the restatement's solve() run of a built case: -> (rr0, checks); the fields are left in B.levels"""
    c = B.case
    return rst.run(B.levels, B.x0, B.b, c["n"], c["pre"], c["post"], c["coarse_sweeps"], c["check_every"])


def expected_counts(case):
    """(plain, graph, checks) of solve() / (plain, graph, checks) of cg_solve for `n` cycles or iterations with no tolerance:
    the first runs as plain launches, and when at least two more may follow one is captured and every later one replays it"""
    n = case["n"]
    plain = n if (not case["graph"] or n < 3) else 1
    return plain, n - plain, -(-n // case["check_every"])


# the seed list: chosen so that tests/test_mgfuzz_host.py's coverage items all hold (a seed taken out fails there)
SEEDS = [0, 5, 38, 41, 49, 67, 71, 82, 95, 102, 122, 123, 166, 191, 222, 266, 276, 291, 293, 299, 308, 352,      # solve
         1006, 1010, 1026, 1057, 1068, 1070, 1092, 1175, 1201, 1350,                                              # cg
         2021, 2023, 2030, 2046, 2056, 2264, 2274, 2296,                                                          # cg-lines
         3006, 3007, 3024, 3047, 3090, 3196, 3225, 3352,                                                          # mixed
         9000, 9001, 9002]                                                                                        # refused


def describe(seed):
    case = decode(seed)
    lines = [f"seed {seed}: {case['form']}" + (f" ({case['why']})" if "why" in case else "") +
             f", template {case['template']}, rank {case['rank']}, {np.dtype(case['dtype']).name}, {case['n_levels']} levels"]
    for l in range(case["n_levels"]):
        pair = f"  -> {case['kinds'][l]} along {case['transferred'][l]}" if l + 1 < case["n_levels"] else ""
        lines.append(f"  level {l}: box {case['shapes'][l]}, bounds {case['bounds'][l]}, Omega {case['m'][l]} at {case['lo'][l]}, "
                     f"region {region_of(case, l)}, weights {case['weights'][l]}, stages {case['stages'][l]}{pair}")
    lines.append("  " + ", ".join(f"{k} = {case[k]}" for k in ("pre", "post", "sweeps", "coarse_sweeps", "n", "check_every", "graph",
                                                               "offset", "both_paths", "tiny")))
    return "\n".join(lines)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--describe":
        print(describe(int(sys.argv[2])))
    else:
        print("usage: python tests/mgfuzz_cases.py --describe SEED")
