"""Record what the multigrid case modules' OWN restatements produce, as exact bits.

Before tests/mg_restatement.py every feature's case module carried its own copy of the cycle, the run, the MGCG
preconditioner and the replay.  This tool runs those copies -- from a checkout of the commit that still has them, given with
--tests DIR -- on fixed small problems and writes tests/golden/mg_restatement.json; tests/test_mgfuzz_host.py holds the one
restatement to these bits.  It runs on the CPU and needs nothing of the product but the oracle.  Against a tests/ directory
that has the one restatement already it cannot run: the functions named in SOLVES and CGS below are gone there.

    git worktree add --detach ../parent <the commit named in the file>
    python tools/record_mg_restatement.py --tests ../parent/tests

Scalars and (sum, bound) pairs are float.hex() strings; a field is the SHA-256 of its bytes with its shape and dtype (the
work fields hold NaN fill: bytes are compared, not values).  The problem tables and the record's layout are shared with the
test, which imports them from here: the builders they call have the same names before and after."""
import argparse
import hashlib
import importlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "mg_restatement.json"
SCHEDULES = ((2, 2, 8, 1), (1, 2, 3, 2))        # (pre, post, coarse_sweeps, check_every) of the solves, CYCLES cycles each
CYCLES, ITERS, SWEEPS, COARSE_SWEEPS = 2, 3, 2, 4
D, S = np.float64, np.float32
DAMP = 0.8
MIXED_FACES = [("neumann", "dirichlet"), ("dirichlet", "dirichlet")]
MIXED_RIM, ODD_RIM = ((0, 1), (1, 1)), ((1, 1), (1, 1))       # the rules of MIXED_FACES and of "dirichlet": EVEN = 0, ODD = 1


def _m(name):
    return importlib.import_module(name)


# ---------------------------------------------------------------- the problems
def _point0_levels():
    levels = _m("mglines_cases").star_levels((7, 15), 3, D, DAMP, [(), (0,), (1, 0)])[0]
    levels[0].minv = _m("mg_cases").minv_field(levels[0].shape, levels[0].where, D, DAMP, outside=0.0)
    return levels


def _halved(pairs=((0, 1), (1,)), omega=(8, 16)):
    cc = _m("mgcc_cases")
    return cc.halved_steps(omega, [cc.Halved(p) for p in pairs])


def _linear_levels(stage=False):
    """a Linear pair with different rules on the two faces of dimension 0; stage: a line stage along 1 on level 1"""
    cc, cl = _m("mgcc_cases"), _m("mgcl_cases")
    levels, _, rests = cl.flux_levels(cl.linear_steps(_halved(((0, 1), (0, 1))), MIXED_RIM), DAMP, D, MIXED_FACES)
    if stage:
        _stage_on_level_1(levels, rests, cl.mixed_face_fields(levels[1].m, D, MIXED_FACES, levels[1].weights)[1])
    return levels


def _stage_on_level_1(levels, rests, diag):
    """the stage's factors from the operator's own coefficient fields, as the modules' solve tests build them"""
    R1, c1 = levels[1], rests[1][1]
    up_coef = np.zeros_like(c1)
    up_coef[:, :-1] = c1[:, 1:]
    R1.stages = [(1,) + _m("mglines_cases").factors(-c1, diag, -up_coef, R1.where, 1, DAMP)]


def _transfer_levels(dtype, prolong="linear", restrict="linear", stage=False):
    cc, cl, cs = _m("mgcc_cases"), _m("mgcl_cases"), _m("mgcs_cases")
    steps = cs.transfer_steps(_halved(((0, 1), (0, 1))), ODD_RIM, prolong, restrict)
    levels, _, rests = cs.flux_levels(steps, DAMP, dtype, "dirichlet")
    if stage:
        _stage_on_level_1(levels, rests, cc.face_fields(levels[1].m, dtype, "dirichlet", levels[1].weights)[1])
    return levels


def _transfer_mixed():
    return _m("mgcgmixed_cases").Problem(_transfer_levels(D)[0].A, _transfer_levels(S))


# name: (make the levels, the old copy's run)
SOLVES = {
    "mg_star": (lambda: _m("mg_cases").star_levels((15, 31), 3, D, DAMP)[0], "mg_cases.run"),
    "mg_star_f32_rank3": (lambda: _m("mg_cases").star_levels((7, 7, 15), 2, S, DAMP)[0], "mg_cases.run"),
    "mgsemi_plan": (lambda: _m("mgsemi_cases").plan_levels((15, 31), (1.0, 16.0), DAMP)[0], "mgsemi_cases.run"),
    "mglines_star": (lambda: _m("mglines_cases").star_levels((7, 15), 3, D, DAMP, [(0, 1), (1,), ()])[0], "mglines_cases.run"),
    "mglines_flux": (lambda: _m("mglines_cases").flux_levels((0, 1), n=17)[0], "mglines_cases.run"),
    "mgcc_flux": (lambda: _m("mgcc_cases").flux_levels(_halved(), DAMP, D, "dirichlet")[0], "mgcc_cases.run"),
    "mgcc_switch": (lambda: _m("mgcc_cases").flux_levels(
        _m("mgcc_cases").halved_steps((14, 14), [_m("mgcc_cases").Halved((0, 1)), (0, 1)]), DAMP, S, "dirichlet")[0], "mgcc_cases.run"),
    # beyond the seven of the former cross-check: what those do not reach
    "mgsemi_rank3_f32_kept_contiguous": (lambda: _m("mgsemi_cases").build_levels(
        _m("mgsemi_cases").with_axes((7, 7, 15), (1.0, 1.0, 1.0), [(0, 1), (0, 1, 2)]), DAMP, S)[0], "mgsemi_cases.run"),
    "mgcl_two_rules": (_linear_levels, "mgcl_cases.run"),
    "mgcl_two_rules_stage": (lambda: _linear_levels(stage=True), "mgcl_cases.lines_run"),
    "mgcs_linear_f64": (lambda: _transfer_levels(D), "mgcs_cases.run"),
    "mgcs_linear_f32": (lambda: _transfer_levels(S), "mgcs_cases.run"),
    "mgcs_constant_prolong_linear_restrict": (lambda: _transfer_levels(D, prolong="constant"), "mgcs_cases.run"),
}

# name: (make the levels or the mixed Problem, the old copy's numpy_mgcg or None, the old copy's replay)
CGS = {
    "mgcg": (lambda: _m("mgcg_cases").star_levels((15, 15), 3, D, DAMP)[0], "mgcg_cases.numpy_mgcg", "mgcg_cases.replay"),
    "mgcg_f32": (lambda: _m("mgcg_cases").star_levels((7, 31), 2, S, DAMP)[0], "mgcg_cases.numpy_mgcg", "mgcg_cases.replay"),
    "mgsemi": (lambda: _m("mgsemi_cases").plan_levels((15, 31), (1.0, 16.0), DAMP)[0], None, "mgsemi_cases.replay"),
    "mgcc": (lambda: _m("mgcc_cases").flux_levels(_halved(), DAMP, D, "dirichlet")[0], "mgcc_cases.numpy_mgcg", "mgcc_cases.replay"),
    "mgcglines": (lambda: _m("mglines_cases").star_levels((7, 15), 3, D, DAMP, [(0, 1), (1,), ()])[0],
                  "mgcglines_cases.numpy_mgcg", "mgcglines_cases.replay"),
    "mgcglines_point0": (_point0_levels, "mgcglines_cases.numpy_mgcg", "mgcglines_cases.replay"),
    "mgcgmixed": (lambda: _m("mgcgmixed_cases").star_problem((15, 15), 3, DAMP)[0],
                  "mgcgmixed_cases.numpy_mgcg_mixed", "mgcgmixed_cases.replay"),
    "mgcs_linear_f64": (lambda: _transfer_levels(D), "mgcs_cases.numpy_mgcg", "mgcs_cases.replay"),
    "mgcs_linear_f32": (lambda: _transfer_levels(S), "mgcs_cases.numpy_mgcg", "mgcs_cases.replay"),
    "mgcs_composed_stage": (lambda: _transfer_levels(D, stage=True), None, "mgcs_cases.composed.replay"),
    "mgcs_composed_mixed": (_transfer_mixed, None, "mgcs_cases.composed.replay"),
}


def levels_of(problem):
    return getattr(problem, "levels", problem)


def problem_fields(problem):
    """x0 (hashed Dirichlet values on the rim, zeros inside) and a hashed b, in the outer element type"""
    L0 = levels_of(problem)[0]
    x0, b = _m("mg_cases").problem_fields(L0.shape, L0.where, L0.dt, rim=True, seed=91)
    return (x0.astype(D), b.astype(D)) if hasattr(problem, "levels") else (x0, b)


# ---------------------------------------------------------------- the record's layout
def digest(a):
    """'<SHA-256 of the bytes> <dtype, as numpy's '<f8'> <extents>' of a field"""
    return f"{hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()} {a.dtype.str} {'x'.join(str(n) for n in a.shape)}"


def hexes(v):
    """a scalar -> its float.hex(); a (nested) sequence of them -> nested lists"""
    if isinstance(v, (tuple, list)):
        return [hexes(x) for x in v]
    return float(v).hex()


def level_fields(levels, names, first=0):
    return {f"{nm}_{l}": digest(getattr(L, nm)) for l, L in enumerate(levels) if l >= first for nm in names}


def solve_record(rr0, checks, levels):
    return {"rr0": hexes(rr0), "checks": hexes(checks), "fields": level_fields(levels, ("x", "b", "q"))}


def cg_record(seq, fields, checks, rr0, rz0, levels):
    """seq: the r . r sequence of numpy_mgcg, [rr_0] + the trace's third column (None where the old copy had none): its head
    is recorded, the trace holds the rest; fields: {name: array} of the replay"""
    return {"numpy_rr0": None if seq is None else hexes(seq[0]), "fields": {nm: digest(a) for nm, a in fields.items()},
            "checks": hexes(checks), "rr0": hexes(rr0), "rz0": hexes(rz0), "levels": level_fields(levels, ("x", "b"), first=1)}


def differences(got, want, path=""):
    """the paths at which two records differ, e.g. '[1]/fields/x_1'"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(got.get(k), want.get(k), f"{path}/{k}")]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{path}[{i}]")]
    return [] if got == want else [f"{path.lstrip('/')}: {got!r} != {want!r}"]


def dumps(doc):
    """the file's text: one line per problem"""
    one = lambda v: json.dumps(v, separators=(",", ":"))
    lines = [f' "{k}":{one(v)}' for k, v in doc.items() if k not in ("solves", "cgs")]
    for group in ("solves", "cgs"):
        lines.append(f' "{group}":{{\n' + ",\n".join(f'  "{k}":{one(v)}' for k, v in doc[group].items()) + "\n }")
    return "{\n" + ",\n".join(lines) + "\n}\n"


# ---------------------------------------------------------------- the old copies, run
def _old(dotted):
    module, _, attr = dotted.partition(".")
    fn = _m(module)
    for part in attr.split("."):
        fn = getattr(fn, part)
    return fn


def record_solve(name):
    make, run = SOLVES[name]
    levels = make()
    x0, b = problem_fields(levels)
    out = []
    for pre, post, cs, every in SCHEDULES:
        rr0, checks = _old(run)(levels, x0, b, CYCLES, pre, post, cs, every)
        out.append(solve_record(rr0, checks, levels))
    return out


def record_cg(name, scalars):
    """scalars: the (rz0, trace rows) that drive the replay -- the composed restatement's with numpy's own sums, which the old
    numpy_mgcg's sequence must equal where there is one"""
    make, numpy_mgcg, replay = CGS[name]
    problem = make()
    x0, b = problem_fields(problem)
    seq = None
    if numpy_mgcg is not None:
        seq = _old(numpy_mgcg)(problem, x0, b, ITERS, SWEEPS, COARSE_SWEEPS)
        seq = seq[0] if isinstance(seq, tuple) else seq
    rz0, trace = scalars(problem, x0, b)
    assert seq is None or [float(row[2]) for row in trace] == seq[1:], name
    out = _old(replay)(problem, x0, b, rz0, trace, SWEEPS, COARSE_SWEEPS)
    names = ("x", "r", "p", "r32", "z32") if hasattr(problem, "levels") else ("x", "r", "p", "z")
    if isinstance(out[0], np.ndarray):
        fields, (checks, rr0, rz0_ref) = dict(zip(names, out)), out[-3:]
    else:                                       # the composed copy: (State, checks, rr0, rz0, scalars)
        fields, (checks, rr0, rz0_ref) = {nm: getattr(out[0], nm) for nm in names}, out[1:4]
    rec = cg_record(seq, fields, checks, rr0, rz0_ref, levels_of(problem))
    rec["rz0_used"], rec["trace"] = hexes(rz0), hexes([list(row) for row in trace])
    return rec


def _composed_scalars(problem, x0, b):
    """the old composed restatement with numpy's own sums: -> (rz0, trace rows (pq, rz', rr'))"""
    fz = _m("mgcs_cases").composed
    st, _, _, _, scalars = fz.replay(problem, x0, b, sweeps=SWEEPS, coarse_sweeps=COARSE_SWEEPS, iters=ITERS)
    assert not any(s[3] for s in scalars)
    return st.rz0_used, np.array([[s[0], s[1], s[2]] for s in scalars])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tests", required=True, type=Path, help="the tests/ directory of a checkout that has the old copies")
    ap.add_argument("--out", type=Path, default=GOLDEN)
    args = ap.parse_args()
    tests = args.tests.resolve()
    assert not (tests / "mg_restatement.py").exists(), "this checkout has the one restatement already: nothing to witness"
    sys.path[:0] = [str(tests), str(tests.parent)]
    commit = subprocess.run(["git", "-C", str(tests), "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    doc = {"recorded_from": commit, "schedules": [list(s) for s in SCHEDULES], "cycles": CYCLES, "iters": ITERS, "sweeps": SWEEPS,
           "coarse_sweeps": COARSE_SWEEPS,
           "solves": {name: record_solve(name) for name in SOLVES},
           "cgs": {name: record_cg(name, _composed_scalars) for name in CGS}}
    args.out.write_text(dumps(doc))
    print(f"{args.out}: {len(doc['solves'])} solves, {len(doc['cgs'])} CG problems from {commit[:12]}, {args.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
