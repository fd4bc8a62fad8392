"""Groups of sibling applies over shared inputs, without a GPU: what the lowering recognises as a group and
what it must not, that the emitted multi-output module cross-compiles for gfx950, that the oracle means what the fixtures
say, and the tuple-returning kernels of the Python front end."""
import numpy as np
import pytest

import group_cases as gc
import helpers
from helpers import bits_equal, oracle

import neptune as nep
from neptune_hip import lowering


@pytest.mark.parametrize("kind", ["swe", "pair"])
def test_fixture_lowers_to_one_group_launch_and_cross_compiles(kind, tmp_path, monkeypatch):
    text = gc.fixture_text(kind)
    lowering.verify(text)
    src, report = lowering.to_hip(text)
    n = gc.NOUT[kind]
    assert src.count("nl::run_apply_group<") == 1 and "nl::run_apply<" not in src
    assert len(report["groups"]) == 1
    grp = report["groups"][0]
    tags = [f"entry_{m}" for m in range(n)]
    assert grp["members"] == tags and grp["function"] == "entry" and grp["kernel"] == "march"
    assert grp["inputs"] == (["%h", "%qx", "%qy"] if kind == "swe" else ["%u", "%v"])
    applies = {a["tag"]: a for a in report["applies"]}
    assert list(applies) == tags
    for tag in tags:
        a = applies[tag]
        assert a["group"] == 0 and a["geom_symbol"] == tag + "__geom" and a["kernel"] == "march" and a["inputs"] == n
        for suffix in ("", "_variants", "2", "3"):
            assert f'extern "C" int {tag}__geom{suffix}(' in src
    # member m lists its own unknown first: the map from member input to group input is part of the group body's type
    want_maps = ["3, 0, 1, 2>", "3, 1, 0, 2>", "3, 2, 0, 1>"] if kind == "swe" else ["2, 0, 1>", "2, 1, 0>"]
    for m, wm in enumerate(want_maps):
        assert f"neptune_hip::GroupMember<Body_entry_{m}, FP_entry_{m}, {wm}" in src
    # every result may be written straight into its field: none of them is an input
    assert "dest_entry_0_group[] = {" + ", ".join("&v_fo" + s for s in (["h", "qx", "qy"] if kind == "swe" else ["u", "v"])) + "}" in src
    monkeypatch.setenv("NEPTUNE_CACHE_DIR", str(tmp_path))
    small = gc.variant(kind, (24, 512) if kind == "swe" else (9, 12, 256))
    mod = lowering.compile_module(small)          # hipcc --offload-arch=gfx950; no device needed
    assert hasattr(mod.lib, "entry") and len(mod.report["groups"]) == 1
    for tag in tags:
        assert hasattr(mod.lib, tag + "__geom")


def _pair(shape=(9, 12, 256)):
    return gc.variant("pair", shape)


def _no_group(text):
    lowering.verify(text)
    src, report = lowering.to_hip(text)
    assert report["groups"] == [] and "run_apply_group" not in src
    assert all("group" not in a for a in report["applies"])
    return src, report


def test_a_store_between_the_members_prevents_the_group():
    text = _pair()
    store = "    neptune_ir.store %ru to %fou : !temp to !field\n"
    assert text.count(store) == 1
    head, tail = text.replace(store, "").split("    %rv = neptune_ir.apply(")
    _no_group(head + store + "    %rv = neptune_ir.apply(" + tail)


def test_a_member_reading_another_members_result_prevents_the_group():
    text = _pair()
    assert text.count("%rv = neptune_ir.apply(%v, %u)") == 1
    _no_group(text.replace("%rv = neptune_ir.apply(%v, %u)", "%rv = neptune_ir.apply(%v, %ru)"))


def test_different_apply_bounds_prevent_the_group():
    text = _pair()
    head, tail = text.split("    %rv = neptune_ir.apply(%v, %u) attributes {bounds = #bi}")
    _no_group(head + "    %rv = neptune_ir.apply(%v, %u) attributes {bounds = #neptune_ir.bounds<lb = [1, 1, 1], ub = [8, 10, 255]>}" + tail)


def test_five_distinct_inputs_prevent_the_group():
    text = _pair()
    loads = "".join(f"    %x{k} = neptune_ir.load %fu : !field -> !temp\n" for k in range(3))
    text = text.replace("    %ru = neptune_ir.apply(", loads + "    %ru = neptune_ir.apply(")
    text = text.replace("%ru = neptune_ir.apply(%u, %v) attributes {bounds = #bi} : (!temp, !temp) -> !temp {\n"
                        "      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp):",
                        "%ru = neptune_ir.apply(%u, %v, %x0) attributes {bounds = #bi} : (!temp, !temp, !temp) -> !temp {\n"
                        "      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp, %e0: !temp):")
    text = text.replace("%rv = neptune_ir.apply(%v, %u) attributes {bounds = #bi} : (!temp, !temp) -> !temp {\n"
                        "      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp):",
                        "%rv = neptune_ir.apply(%v, %u, %x1, %x2) attributes {bounds = #bi} : (!temp, !temp, !temp, !temp) -> !temp {\n"
                        "      ^bb0(%i0: index, %i1: index, %i2: index, %a: !temp, %o: !temp, %e1: !temp, %e2: !temp):")
    assert "%x0)" in text and "%x2)" in text
    _, report = _no_group(text)
    assert [a["inputs"] for a in report["applies"]] == [3, 4]
    # four distinct values are still one group
    four = text.replace("(%v, %u, %x1, %x2)", "(%v, %u, %x1, %x0)")
    assert len(lowering.to_hip(four)[1]["groups"]) == 1


def test_an_input_0_in_a_larger_box_prevents_the_group():
    """%v lives in a box one plane larger; member 1 lists it first, so its input 0 (and its result) are not in member 0's
    result box, and the centre of the group input would not be 'the same physical index'"""
    text = _pair()
    big = "!tbig = !neptune_ir.temp<element = f64, bounds = #neptune_ir.bounds<lb = [0, 0, 0], ub = [10, 12, 256]>, location = #loc>\n"
    text = text.replace("module {", big + "module {", 1)
    text = text.replace("%v   = neptune_ir.load %fv : !field -> !temp", "%v   = neptune_ir.load %fv : !field -> !tbig")
    head, rest = text.split("    %ru = neptune_ir.apply(")
    m0, rest = rest.split("    %rv = neptune_ir.apply(")
    m1, tail = rest.split("    neptune_ir.store %ru")
    m0 = m0.replace("(!temp, !temp) -> !temp", "(!temp, !tbig) -> !temp").replace("%o: !temp", "%o: !tbig")
    m0 = m0.replace("%o[0, 0, 0] : !temp", "%o[0, 0, 0] : !tbig")
    m1 = m1.replace("!temp", "!tbig").replace("(!tbig, !tbig) -> !tbig", "(!tbig, !temp) -> !tbig").replace("%o: !tbig", "%o: !temp")
    m1 = m1.replace("%o[0, 0, 0] : !tbig", "%o[0, 0, 0] : !temp")
    tail = tail.replace("neptune_ir.store %rv to %fov : !temp to !field", "neptune_ir.store %rv to %fov {bounds = #b} : !tbig to !field")
    text = head + "    %ru = neptune_ir.apply(" + m0 + "    %rv = neptune_ir.apply(" + m1 + "    neptune_ir.store %ru" + tail
    src, report = lowering.to_hip(text)      # (only the lowering's view is asked for: a load into a larger box cannot run)
    assert report["groups"] == [] and "run_apply_group" not in src and len(report["applies"]) == 2


def test_oracle_computes_what_the_fixtures_say():
    """the yardstick of the GPU tests, checked against cells evaluated by hand: same operations, same order"""
    shape = (7, 9)
    h, qx, qy = gc.inputs("swe", shape, np.float64)
    oh, oqx, oqy = gc.oracle_run(gc.variant("swe", shape, [2, 1], [6, 7]), shape, np.float64, [h, qx, qy])
    a, nu, g2 = 0.125, 0.03125, 0.5
    for (i, j) in [(2, 1), (3, 4), (5, 6)]:
        adv = a * ((qx[i + 1, j] - qx[i - 1, j]) + (qy[i, j + 1] - qy[i, j - 1]))
        lap = (((h[i - 1, j] + h[i + 1, j]) + h[i, j - 1]) + h[i, j + 1]) - 4.0 * h[i, j]
        assert oh[i, j] == (h[i, j] - adv) + nu * lap

        def flux(m, hh):
            return m * (m / hh) + g2 * (hh * hh)
        df = flux(qx[i + 1, j], h[i + 1, j]) - flux(qx[i - 1, j], h[i - 1, j])
        dg = qx[i, j + 1] * (qy[i, j + 1] / h[i, j + 1]) - qx[i, j - 1] * (qy[i, j - 1] / h[i, j - 1])
        assert oqx[i, j] == qx[i, j] - a * (df + dg)
        df = flux(qy[i, j + 1], h[i, j + 1]) - flux(qy[i, j - 1], h[i, j - 1])
        dg = qy[i + 1, j] * (qx[i + 1, j] / h[i + 1, j]) - qy[i - 1, j] * (qx[i - 1, j] / h[i - 1, j])
        assert oqy[i, j] == qy[i, j] - a * (df + dg)
    # outside apply.bounds every result is ITS OWN unknown: a different copy-through source per member
    for got, src in ((oh, h), (oqx, qx), (oqy, qy)):
        assert bits_equal(got[:2], src[:2]) and bits_equal(got[:, 7:], src[:, 7:]) and bits_equal(got[6:], src[6:])
    shape = (5, 6, 8)
    u, v = gc.inputs("pair", shape, np.float64)
    ou, ov = gc.oracle_run(gc.variant("pair", shape), shape, np.float64, [u, v])

    def lap7(f, i, j, k):
        s = ((((f[i - 1, j, k] + f[i + 1, j, k]) + f[i, j - 1, k]) + f[i, j + 1, k]) + f[i, j, k - 1]) + f[i, j, k + 1]
        return 0.0625 * (s - 6.0 * f[i, j, k])
    for (i, j, k) in [(1, 1, 1), (2, 3, 5), (3, 4, 6)]:
        assert ou[i, j, k] == u[i, j, k] + 0.25 * (lap7(u, i, j, k) - v[i, j, k])
        assert ov[i, j, k] == v[i, j, k] + 0.25 * (lap7(v, i, j, k) + u[i, j, k])
    assert bits_equal(ou[0], u[0]) and bits_equal(ov[0], v[0]) and bits_equal(ov[:, :, 7], v[:, :, 7])
    # the band helper of the GPU tests reproduces the rows of the whole problem
    shape, lb, ub = (12, 9), [2, 1], [11, 7]
    ins = gc.inputs("swe", shape, np.float64)
    whole = gc.oracle_run(gc.variant("swe", shape, lb, ub), shape, np.float64, ins)
    for g0, g1 in ((0, 3), (4, 7), (9, 12)):
        for w, b in zip(whole, gc.oracle_band("swe", shape, lb, ub, np.float64, ins, g0, g1)):
            assert bits_equal(np.ascontiguousarray(w[g0:g1]), np.ascontiguousarray(b))


@pytest.fixture
def fresh_module():
    nep.reset()
    yield
    nep.reset()


def _system(through, n0=8, n1=12):
    box = ([0, 0], [n0, n1])
    c = nep.get_compiler()
    c.start_function("step", [("memref", 2)] * 4)
    fo = [nep.wrap(nep.Expr(c.get_function_arg(i)), box) for i in (0, 1)]
    h, q = (nep.load(nep.wrap(nep.Expr(c.get_function_arg(i)), box)) for i in (2, 3))
    kw = {} if through is None else {"through": through}

    @nep.apply(inputs=[h, q], bounds=([1, 1], [n0 - 1, n1 - 1]), **kw)
    def resid(h, q):
        res_h = h[0, 0] - (q[1, 0] - q[-1, 0]) * 0.25
        res_q = q[0, 0] - (q[0, 1] / h[0, 1] - q[0, -1] / h[0, -1]) * 0.5
        return res_h, res_q

    assert isinstance(resid, tuple) and len(resid) == 2 and all(isinstance(r, nep.Expr) for r in resid)
    for r, f in zip(resid, fo):
        nep.store(r, f)
    c.create_return(nep.unwrap(fo[0])._handle)
    c.end_function()
    return c.dump()


@pytest.mark.parametrize("through", [None, (0, 1)])
def test_tuple_returning_kernel_makes_one_apply_per_element(fresh_module, through):
    n0, n1 = 8, 12
    text = _system(through, n0, n1)
    lowering.verify(text)
    applies = [ln for ln in text.splitlines() if "= neptune_ir.apply(" in ln]
    assert len(applies) == 2 and text.count("neptune_ir.yield") == 2
    operands = [ln.split("neptune_ir.apply(")[1].split(")")[0].split(", ") for ln in applies]
    assert sorted(operands[0]) == sorted(operands[1])                                # the same operands ...
    assert operands[1] == (operands[0] if through is None else operands[0][::-1])    # ... member 1's own unknown first
    assert len({ln.split("attributes")[1] for ln in applies}) == 1                   # ... and the same bounds
    # each region holds only what its own value needs: no division in member 0, a single yield each
    regions = text.split("= neptune_ir.apply(")[1:]
    assert "arith.divf" not in regions[0].split("neptune_ir.yield")[0] and "arith.divf" in regions[1].split("neptune_ir.yield")[0]
    src, report = lowering.to_hip(text)
    assert len(report["groups"]) == 1 and report["groups"][0]["members"] == ["step_0", "step_1"]
    assert src.count("nl::run_apply_group<") == 1
    # ... and it means what the DSL says
    h = (helpers.hash_field((n0, n1), np.float64, seed=3) * 0.25 + 1.5)
    q = helpers.hash_field((n0, n1), np.float64, seed=4)
    oh, oq = np.zeros_like(h), np.zeros_like(q)
    oracle.Module.parse(text).call("step", oh, oq, h, q)
    want_h, want_q = h.copy(), (q if through else h).copy()
    want_h[1:-1, 1:-1] = h[1:-1, 1:-1] - (q[2:, 1:-1] - q[:-2, 1:-1]) * 0.25
    want_q[1:-1, 1:-1] = q[1:-1, 1:-1] - (q[1:-1, 2:] / h[1:-1, 2:] - q[1:-1, :-2] / h[1:-1, :-2]) * 0.5
    assert bits_equal(oh, want_h) and bits_equal(oq, want_q)


def test_through_is_checked(fresh_module):
    with pytest.raises(ValueError):
        _system((0, 1, 1))
    nep.reset()
    with pytest.raises(ValueError):
        _system((0, 2))


def test_single_expr_kernel_builds_the_text_it_always_built(fresh_module):
    """recorded from the commit before tuple results existed (dead code in the region included: nothing is pruned)"""
    box = ([0, 0], [10, 16])
    c = nep.get_compiler()
    c.start_function("blend", [("memref", 2), ("memref", 2), ("memref", 2)])
    fo = nep.wrap(nep.Expr(c.get_function_arg(0)), box)
    a, b = (nep.load(nep.wrap(nep.Expr(c.get_function_arg(i)), box)) for i in (1, 2))

    @nep.apply(inputs=[a, b], bounds=([1, 1], [9, 15]))
    def blend(x, y):
        unused = y[0, 1] * 3.0          # noqa: F841  dead code stays in the region, as traced
        return (x[-1, 0] + x[1, 0]) * 0.5 - y[0, 0] / (x[0, 0] + 2.0)

    assert isinstance(blend, nep.Expr)
    nep.store(blend, fo)
    c.create_return(nep.unwrap(fo)._handle)
    c.end_function()
    assert c.dump() == (helpers.GOLDEN_DIR / "frontend_single_expr_apply.mlir").read_text()
