"""neptune_hip_mg_*  without a GPU: the exports and signatures, every refusal on host pointers (the argument
checks run before the device is touched), the restatement's transfer operators against dense matrices, and the convergence
preconditions the GPU stop tests rely on -- conditions on the restatement (tests/mg_restatement.py), not on the code under test."""
import ctypes as C

import numpy as np
import pytest

import mg_cases as mgc
import mg_restatement as rst
from neptune_hip import _capi
from neptune_hip.geometry import make_geom


@pytest.fixture(scope="module")
def lib(built_libs):
    return _capi.load()


# ---------------------------------------------------------------- exports and signatures
def test_exports_and_signatures(lib):
    names = ["neptune_hip_mg_smooth", "neptune_hip_mg_restrict", "neptune_hip_mg_prolong_add", "neptune_hip_mg_solve",
             "neptune_hip_mg_counts"]
    header = _capi.HEADER_PATH.read_text()
    for name in names:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f"{name}(" in header
    assert len(_capi.SIGNATURES["neptune_hip_mg_solve"][1]) == 15
    assert len(_capi.SIGNATURES["neptune_hip_mg_restrict"][1]) == 9
    plain, graph, checks = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    lib.neptune_hip_mg_counts(C.byref(plain), C.byref(graph), C.byref(checks))
    assert min(plain.value, graph.value, checks.value) >= 0
    lib.neptune_hip_mg_counts(None, None, None)


def test_level_struct_layout_matches_the_header(lib, tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "neptune_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(neptune_hip_mg_level_t), offsetof(neptune_hip_mg_level_t, body),
         offsetof(neptune_hip_mg_level_t, g), offsetof(neptune_hip_mg_level_t, in_rest), offsetof(neptune_hip_mg_level_t, minv),
         offsetof(neptune_hip_mg_level_t, x), offsetof(neptune_hip_mg_level_t, b), offsetof(neptune_hip_mg_level_t, q),
         offsetof(neptune_hip_mg_level_t, rscale));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", str(_capi.REPO_ROOT / "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    L = _capi.MgLevel
    assert got == [C.sizeof(L), L.body.offset, L.g.offset, L.in_rest.offset, L.minv.offset, L.x.offset, L.b.offset, L.q.offset,
                   L.rscale.offset]


# ---------------------------------------------------------------- refusals on host pointers
SHAPES = [(9, 17, 33), (5, 9, 17)]      # Omega 7 x 15 x 31 -> 3 x 7 x 15


class HostHierarchy:
    """two levels of host memory: nothing may ever be launched on it"""

    def __init__(self, shapes=SHAPES, dtype=np.float64):
        self.arrays = [[np.zeros(s, dtype) for _ in range(4)] for s in shapes]     # x, b, q, minv per level
        self.levels = (_capi.MgLevel * len(shapes))()
        for l, s in enumerate(shapes):
            box = ([0] * len(s), list(s))
            L = self.levels[l]
            L.fn, L.body = None, _capi.BODY_LAP3D7_F64
            L.g = make_geom(box, ([1] * len(s), [n - 1 for n in s]))
            x, b, q, minv = (a.ctypes.data for a in self.arrays[l])
            L.x, L.b, L.q, L.minv, L.rscale = x, b, q, minv, 4.0

    def solve(self, lib, n_levels=None, dtype=_capi.F64, pre=2, post=2, coarse=8, max_cycles=4, check_every=1):
        done, rr0, last = C.c_int64(-1), C.c_double(-1.0), C.c_double(-1.0)
        rc = lib.neptune_hip_mg_solve(self.levels, len(self.levels) if n_levels is None else n_levels, dtype, pre, post, coarse,
                                      max_cycles, check_every, 0.0, None, None, None, C.byref(done), C.byref(rr0), C.byref(last))
        assert (done.value, rr0.value, last.value) == (0, 0.0, 0.0)
        return rc


def _refused(lib, change, **kw):
    h = HostHierarchy()
    change(h)
    return h.solve(lib, **kw) == _capi.EINVAL


def test_solve_refusals_on_host_pointers(lib):
    nothing = lambda h: None
    assert _refused(lib, nothing, n_levels=0)
    assert _refused(lib, nothing, n_levels=17)
    assert _refused(lib, nothing, dtype=7)
    assert _refused(lib, nothing, pre=-1)
    assert _refused(lib, nothing, post=-1)
    assert _refused(lib, nothing, coarse=-1)
    assert _refused(lib, nothing, check_every=0)
    assert _refused(lib, nothing, max_cycles=-1)
    assert _refused(lib, nothing, dtype=_capi.F32)                   # the built-in body is an f64 one
    for field in ("x", "b", "q", "minv"):
        for level in (0, 1):
            assert _refused(lib, lambda h: setattr(h.levels[level], field, None)), (field, level)

    def rank_differs(h):
        h.levels[1].g = make_geom(([0, 0], [9, 17]), ([1, 1], [8, 16]))
    assert _refused(lib, rank_differs)
    for d in range(3):
        def size_relation(h, d=d):
            ub = [n - 1 for n in SHAPES[1]]
            ub[d] -= 1
            h.levels[1].g = make_geom(([0] * 3, list(SHAPES[1])), ([1] * 3, ub))
        assert _refused(lib, size_relation), d

    def empty_omega(h):
        h.levels[0].g = make_geom(([0] * 3, list(SHAPES[0])), ([1, 1, 1], [1, 16, 32]))
    assert _refused(lib, empty_omega)

    def empty_region(h):
        h.levels[0].g = make_geom(([0] * 3, list(SHAPES[0])), ([1] * 3, [n - 1 for n in SHAPES[0]]), region=([0, 0, 0], [1, 17, 33]))
    assert _refused(lib, empty_region)

    def input0_box(h):
        s = SHAPES[0]
        h.levels[0].g = make_geom(([0] * 3, list(s)), ([1] * 3, [n - 1 for n in s]), [([1, 0, 0], [s[0] + 1, s[1], s[2]])])
    assert _refused(lib, input0_box)
    for a, b in (("x", "b"), ("x", "q"), ("x", "minv"), ("b", "q"), ("b", "minv"), ("q", "minv")):
        for level in (0, 1):
            assert _refused(lib, lambda h: setattr(h.levels[level], a, getattr(h.levels[level], b) + 8)), (a, b, level)
    for a in ("x", "b", "q", "minv"):
        for b in ("x", "b", "q", "minv"):
            assert _refused(lib, lambda h: setattr(h.levels[1], a, getattr(h.levels[0], b) + 64)), (a, b)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _refused(lib, lambda h: setattr(h.levels[0], "rscale", bad))

    def missing_fixed_input(h):
        s = SHAPES[0]
        box = ([0] * 3, list(s))
        h.levels[0].g = make_geom(box, ([1] * 3, [n - 1 for n in s]), [box, box])
    assert _refused(lib, missing_fixed_input)
    assert _refused(lib, lambda h: setattr(h.levels[0], "body", 99))
    # a null hierarchy
    assert lib.neptune_hip_mg_solve(None, 1, _capi.F64, 2, 2, 8, 4, 1, 0.0, None, None, None, None, None, None) == _capi.EINVAL


def test_kernel_entry_refusals_on_host_pointers(lib):
    h = HostHierarchy()
    (xf, bf, qf, mf), (xc, bc, qc, mc_) = [[a.ctypes.data for a in lvl] for lvl in h.arrays]
    gf, gc = C.byref(h.levels[0].g), C.byref(h.levels[1].g)
    E = _capi.EINVAL
    assert lib.neptune_hip_mg_smooth(7, gf, qf, bf, mf, xf, None) == E
    assert lib.neptune_hip_mg_smooth(_capi.F64, None, qf, bf, mf, xf, None) == E
    for args in ((None, bf, mf, xf), (qf, None, mf, xf), (qf, bf, None, xf), (qf, bf, mf, None), (xf, bf, mf, xf), (qf, xf + 8, mf, xf),
                 (qf, bf, xf, xf)):
        assert lib.neptune_hip_mg_smooth(_capi.F64, gf, *args, None) == E, args
    assert lib.neptune_hip_mg_restrict(_capi.F64, gf, gf, bf, qf, 4.0, bc, xc, None) == E            # the size relation
    assert lib.neptune_hip_mg_restrict(_capi.F64, gf, gc, bf, qf, float("nan"), bc, xc, None) == E
    assert lib.neptune_hip_mg_restrict(_capi.F64, gf, gc, bf, qf, 4.0, bc, bc, None) == E
    assert lib.neptune_hip_mg_restrict(_capi.F64, gf, gc, bf, qf, 4.0, bf, xc, None) == E
    assert lib.neptune_hip_mg_restrict(_capi.F64, gf, gc, None, qf, 4.0, bc, xc, None) == E
    assert lib.neptune_hip_mg_restrict(3, gf, gc, bf, qf, 4.0, bc, xc, None) == E
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, gc, gf, xc, xf, None) == E                       # the size relation
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, gf, gc, xf, xf, None) == E
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, gf, gc, None, xf, None) == E
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, gf, None, xc, xf, None) == E
    g2 = make_geom(([0, 0], [9, 17]), ([1, 1], [8, 16]))
    assert lib.neptune_hip_mg_prolong_add(_capi.F64, gf, C.byref(g2), xc, xf, None) == E              # ranks differ


def test_python_layer_checks(lib):
    from neptune_hip import multigrid
    assert multigrid.coarsen_bounds(([1, 1, 1], [8, 16, 264])) == [3, 7, 131]
    assert multigrid.coarsen_bounds(([0], [3])) == [1]
    with pytest.raises(ValueError, match="dimension 1"):
        multigrid.coarsen_bounds(([1, 1], [8, 15]))
    with pytest.raises(ValueError):
        multigrid.coarsen_bounds(([1], [2]))


# ---------------------------------------------------------------- the restatement's transfer operators, dense
def _dense(f, n_in, n_out):
    M = np.zeros((n_out, n_in))
    for j in range(n_in):
        e = np.zeros(n_in)
        e[j] = 1.0
        M[:, j] = f(e)
    return M


def test_transfer_operators_on_a_seven_cell_line():
    whole = lambda n: (slice(0, n),)
    R = _dense(lambda d: rst.restrict(d, np.zeros(7), whole(7), 1.0, np.full(3, np.nan), np.full(3, np.nan), whole(3))[0], 7, 3)
    want = np.zeros((3, 7))
    for j in range(3):
        want[j, 2 * j:2 * j + 3] = (0.25, 0.5, 0.25)
    assert np.array_equal(R, want)
    P = _dense(lambda e: rst.prolong_add(e, whole(3), np.zeros(7), whole(7)), 3, 7)
    assert np.array_equal(P, 2.0 * R.T)
    # constants are reproduced away from the rim: restriction everywhere (all its operands lie inside), prolongation on
    # every fine cell but the two next to the rim, which interpolate against the rim's zero
    assert np.array_equal(R @ np.ones(7), np.ones(3))
    assert np.array_equal((P @ np.ones(3))[1:-1], np.ones(5)) and P[0, 0] == 0.5 and P[-1, -1] == 0.5
    # restriction writes x = +0 on the coarse Omega and leaves everything outside alone
    bc, xc = rst.restrict(np.ones(9), np.zeros(9), (slice(1, 8),), 4.0, np.full(6, 7.0), np.full(6, 7.0), (slice(2, 5),))
    assert np.array_equal(bc, [7, 7, 4, 4, 4, 7]) and np.array_equal(xc, [7, 7, 0, 0, 0, 7])


def test_tensor_product_matches_the_axis_by_axis_form():
    rng = np.random.default_rng(5)
    e = rng.standard_normal((1, 3, 7))
    out = rst.prolong_add(e, (slice(0, 1), slice(0, 3), slice(0, 7)), np.zeros((3, 7, 15)), (slice(0, 3), slice(0, 7), slice(0, 15)))
    P = [2.0 * _dense(lambda d, n=n: rst.restrict(d, np.zeros(2 * n + 1), (slice(0, 2 * n + 1),), 1.0, np.zeros(n), np.zeros(n),
                                                 (slice(0, n),))[0], 2 * n + 1, n).T for n in (1, 3, 7)]
    want = np.einsum("ai,bj,ck,ijk->abc", P[0], P[1], P[2], e)
    assert np.allclose(out, want, rtol=1e-14, atol=1e-14)
    # m = 1 along dimension 0: both even fine planes interpolate against the +0 rim on both sides
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[0], 0.5 * out[1])


# ---------------------------------------------------------------- convergence preconditions of the GPU stop tests
CONVERGENCE = {
    # name: (Omega, levels, omega, dtype, cycles)
    "3d_f64": ((7, 15, 263), 3, 6.0 / 7.0, np.float64, 6),
    "2d_f64": ((15, 263), 3, 0.8, np.float64, 6),
    "3d_f32": ((7, 15, 263), 3, 6.0 / 7.0, np.float32, 3),
    "2d_f32": ((15, 263), 3, 0.8, np.float32, 3),
}


@pytest.mark.parametrize("name", sorted(CONVERGENCE))
def test_rr_falls_by_a_factor_of_four_per_cycle(name, built_libs):
    omega, n_levels, damp, dtype, cycles = CONVERGENCE[name]
    levels, _ = mgc.star_levels(omega, n_levels, dtype, damp)
    x0, b = mgc.problem_fields(levels[0].shape, levels[0].where, dtype)
    seq = rst.rr_sequence(levels, x0, b, cycles)
    print(name, [f"{a / c:.1f}" for a, c in zip(seq, seq[1:])])
    assert len(seq) == cycles + 1
    for a, c in zip(seq, seq[1:]):
        assert c * 4.0 <= a, seq
