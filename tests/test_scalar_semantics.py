"""Scalar semantics of every op an apply body may contain, on IEEE edge values, without a GPU: the oracle against the
independent model in scalar_spec.py (every op x type x value pair of its tables), the text the HIP emitter produces for
the ops whose C spelling is easy to get wrong, and the oracle's elementary functions (numpy) against a 120-bit
reference."""
import re

import numpy as np
import pytest

import scalar_cases as SC
import scalar_spec as S
from helpers import oracle

# largest error of numpy's elementary functions (the oracle's) over the grids of scalar_cases._grid, in ulps of the
# correctly rounded result: the measured maximum rounded up to a whole ulp
NUMPY_ULP = {
    "f64": {"math.exp": 1, "math.log": 1, "math.sin": 1, "math.cos": 1, "math.tanh": 1, "math.powf": 1},
    "f32": {"math.exp": 2, "math.log": 3, "math.sin": 2, "math.cos": 2, "math.tanh": 1, "math.powf": 1},
}


def _family(fam, ty):
    return SC.float_cases(ty) if fam == "float" else SC.int_cases()


@pytest.mark.parametrize("fam,ty", [("float", "f64"), ("float", "f32"), ("int", "f64")])
def test_oracle_matches_the_spec_on_every_op_and_value_pair(fam, ty):
    cases = _family(fam, ty)
    shape = SC.layout(cases, 2)
    text = SC.module_text(cases, ty, shape)
    ins, expect = SC.fields(cases, ty, shape)
    got = oracle.Module.parse(text).call("ops", *ins)
    n, report = SC.check(got, expect, cases, ty)
    assert n > 20000 and not report, report


def test_spec_pins_the_cases_the_oracle_got_wrong():
    """the spec itself, on the values named in MLIR / LangRef"""
    f64 = S.F64
    pz, nz = S.bits(0.0, f64), S.bits(-0.0, f64)
    assert S.maximumf(0.0, -0.0, f64).bits == {pz} and S.maximumf(-0.0, 0.0, f64).bits == {pz}
    assert S.minimumf(0.0, -0.0, f64).bits == {nz} and S.minimumf(-0.0, 0.0, f64).bits == {nz}
    assert S.maxnumf(0.0, -0.0, f64).bits == {pz, nz}
    assert S.maxnumf(float("nan"), 2.0, f64).bits == {S.bits(2.0, f64)}
    assert S.uitofp(S.wrap(-1, "i32"), "i32", f64).bits == {S.bits(4294967295.0, f64)}
    assert S.uitofp(S.wrap(-1, "i64"), "i64", f64).bits == {S.bits(2.0**64, f64)}
    assert S.sitofp(1, "i1", f64).bits == {S.bits(-1.0, f64)}
    assert S.sitofp(2**24 + 1, "i64", S.F32).bits == {S.bits(2.0**24, S.F32)}          # tie to even, one rounding
    assert S.sitofp(2**60 + 3 * 2**36, "i64", S.F32).bits == {S.bits(2.0**60 + 2**38, S.F32)}
    assert S.addi(2**63 - 1, 1, "i64") == 2**63 and S.addi(1, 1, "i1") == 0
    assert S.cmpi("slt", 1, 0, "i1") and not S.cmpi("ult", 1, 0, "i1")
    assert [p for p in S.CMPF_PREDICATES if S.cmpf(p, float("nan"), 1.0)] == ["ueq", "ugt", "uge", "ult", "ule", "une", "uno"]
    assert S.truncf(float.fromhex("0x1.ffffffp+127")).bits == {S.bits(float("inf"), S.F32)}
    assert S.fptosi(2.0**31, f64, "i32") is S.POISON and S.fptosi(-2.0**31, f64, "i32") == 2**31


# ---- emitted HIP text ------------------------------------------------------------------------------------------------
def _body(lines, ty="f64", extra_inputs=()):
    return ('#l = #neptune_ir.location<"cell">\n'
            f"!t = !neptune_ir.temp<element = {ty}, bounds = #neptune_ir.bounds<lb = [0], ub = [64]>, location = #l>\n"
            "module {\n  neptune_ir.nonlinear_opdef @op : (!t) -> !t {\n  ^bb0(%u: !t):\n"
            "    %r = neptune_ir.apply(%u) attributes {bounds = #neptune_ir.bounds<lb = [0], ub = [64]>} : (!t) -> !t {\n"
            f"      ^bb0(%i: index, %a: !t):\n        %x = neptune_ir.access %a[0] : !t -> {ty}\n"
            + "".join(f"        {l}\n" for l in lines)
            + "    }\n    neptune_ir.return %r : !t\n  }\n}\n")


def _emit(lines, ty="f64"):
    from neptune_hip import lowering
    src, _ = lowering.to_hip(_body(lines, ty))
    return src


def test_uitofp_reads_the_source_width_unsigned(built_libs):
    src = _emit(["%w = arith.index_cast %i : index to i32", "%v = arith.uitofp %w : i32 to f64",
                 "%w64 = arith.index_cast %i : index to i64", "%v64 = arith.uitofp %w64 : i64 to f64",
                 "%b = arith.cmpi slt, %w, %w : i32", "%vb = arith.uitofp %b : i1 to f64",
                 "%s = arith.addf %v, %v64 : f64", "%t = arith.addf %s, %vb : f64", "neptune_ir.yield %t : f64"])
    assert "v_v = (double)(uint32_t)v_w;" in src
    assert "v_v64 = (double)(uint64_t)v_w64;" in src
    assert "v_vb = (double)(bool)v_b;" in src


@pytest.mark.parametrize("ity", ["i32", "i64", "index", "i1"])
def test_integer_arithmetic_wraps_instead_of_overflowing_a_signed_type(built_libs, ity):
    conv = (["%w = arith.index_cast %i : index to i64", f"%a = arith.trunci %w : i64 to {ity}"] if ity in ("i32", "i1")
            else [f"%a = arith.index_cast %i : index to {ity}"])
    out = (["%o = arith.select %m, %x, %x : f64"] if ity == "i1" else
           ["%m64 = arith.index_cast %m : index to i64", "%o = arith.sitofp %m64 : i64 to f64"] if ity == "index" else
           [f"%o = arith.sitofp %m : {ity} to f64"])
    src = _emit(conv + [f"%s = arith.addi %a, %a : {ity}", f"%d = arith.subi %s, %a : {ity}", f"%m = arith.muli %d, %s : {ity}"]
                + out + ["neptune_ir.yield %o : f64"])
    u = "uint64_t" if ity in ("i64", "index") else "uint32_t"
    for name, sym, a, b in (("s", "+", "a", "a"), ("d", "-", "s", "a"), ("m", "*", "d", "s")):
        line = re.search(rf"v_{name} = ([^;]*);", src).group(1)
        assert f"({u})v_{a} {sym} ({u})v_{b}" in line, line
        if ity == "i1":
            assert line.endswith("& 1u) != 0"), line
        else:
            assert line.startswith(f"({SC_CTYPE[ity]})({u})("), line


SC_CTYPE = {"i32": "int32_t", "i64": "int64_t", "index": "int64_t"}

CMPF_TEXT = {"oeq": "v_x == v_y", "ogt": "v_x > v_y", "oge": "v_x >= v_y", "olt": "v_x < v_y", "ole": "v_x <= v_y",
             "one": "(v_x < v_y || v_x > v_y)", "ord": "(v_x == v_x && v_y == v_y)", "ueq": "!(v_x < v_y || v_x > v_y)",
             "ugt": "!(v_x <= v_y)", "uge": "!(v_x < v_y)", "ult": "!(v_x >= v_y)", "ule": "!(v_x > v_y)",
             "une": "v_x != v_y", "uno": "(v_x != v_x || v_y != v_y)"}


@pytest.mark.parametrize("pred", S.CMPF_PREDICATES)
def test_cmpf_predicates_emit_nan_correct_expressions(built_libs, pred):
    """the C comparison operators are false on NaN, so an unordered predicate is the negation of the opposite ordered
    relation; the GPU suite evaluates each on every value pair (test_scalar_ops_gpu.py)"""
    src = _emit(["%y = arith.negf %x : f64", f"%c = arith.cmpf {pred}, %x, %y : f64", "%o = arith.select %c, %x, %y : f64",
                 "neptune_ir.yield %o : f64"])
    assert f"const bool v_c = {CMPF_TEXT[pred]};" in src


def test_signed_i1_compares_and_extensions_read_true_as_minus_one(built_libs):
    src = _emit(["%w = arith.index_cast %i : index to i64", "%b = arith.trunci %w : i64 to i1",
                 "%c = arith.cmpi slt, %b, %b : i1", "%e = arith.extsi %b : i1 to i64", "%f = arith.sitofp %b : i1 to f64",
                 "%o = arith.select %c, %x, %f : f64", "neptune_ir.yield %o : f64"])
    assert "v_b = (((uint64_t)v_w) & 1u) != 0;" in src
    assert "v_c = (-(int64_t)v_b) < (-(int64_t)v_b);" in src
    assert "v_e = (int64_t)(-(int64_t)v_b);" in src and "v_f = (double)(-(int64_t)v_b);" in src


@pytest.mark.parametrize("ty,lit,value", [("f64", "0x7FF0000000000000", float("inf")), ("f64", "0xFFF0000000000000", -float("inf")),
                                          ("f64", "0x8000000000000000", -0.0), ("f32", "0x7F800000", float("inf")),
                                          ("f32", "0xFF800000", -float("inf")), ("f32", "0x80000000", -0.0)])
def test_hex_float_constants_lower_as_bit_patterns(built_libs, ty, lit, value):
    lines = [f"%k = arith.constant {lit} : {ty}", f"%o = arith.mulf %x, %k : {ty}", f"neptune_ir.yield %o : {ty}"]
    src = _emit(lines, ty)
    u = "uint64_t" if ty == "f64" else "uint32_t"
    assert f"__builtin_bit_cast({'double' if ty == 'f64' else 'float'}, ({u}){lit}ull)" in src
    # and the oracle reads the same bits
    k = oracle.Module.parse(_body(lines, ty)).call("op", np.ones(64, dtype=SC.NP[ty]))
    assert S.bits(float(k[0]), ty) == S.bits(value, ty)


def test_hex_nan_constant_through_the_oracle():
    for ty, lit in (("f64", "0x7FF8000000000000"), ("f32", "0x7FC00000"), ("f64", "0xFFF8000000000000")):
        got = oracle.Module.parse(_body([f"%k = arith.constant {lit} : {ty}", f"neptune_ir.yield %k : {ty}"], ty)).call(
            "op", np.zeros(64, dtype=SC.NP[ty]))
        assert S.bits(float(got[3]), ty) == int(lit, 16) or S.is_nan_bits(int(got.view(SC.UINT[ty])[3]), ty)


@pytest.mark.parametrize("ty,lit", [("f64", "0x7F800000"), ("f32", "0x7FF0000000000000"), ("f64", "0x7FF00000000000000"), ("f32", "0x7F8000"), ("f64", "-0x8000000000000000")])
def test_hex_float_constants_of_the_wrong_width_are_refused(built_libs, ty, lit):
    from neptune_hip import lowering
    with pytest.raises(lowering.LoweringError, match="hex constant is the bit pattern"):
        lowering.to_hip(_body([f"%k = arith.constant {lit} : {ty}", f"neptune_ir.yield %k : {ty}"], ty))


# ---- elementary functions: the oracle (numpy) against 120 bits ------------------------------------------------------
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_oracle_elementary_functions_against_a_120_bit_reference(ty):
    """the same grids and special values the GPU suite runs on the device: when the device and the oracle disagree,
    this shows which side is off"""
    pytest.importorskip("mpmath")
    cases = SC.elementary_cases(ty)
    shape = SC.layout(cases, 2)
    got = oracle.Module.parse(SC.module_text(cases, ty, shape)).call("ops", *SC.elementary_fields(cases, ty, shape))
    worst, bad = SC.elementary_check(got, cases, ty, shape)
    assert not bad, "\n".join(bad)
    over = {f: w for f, w in worst.items() if w > NUMPY_ULP[ty][f]}
    assert not over, f"numpy {ty}: ulp error above the bound: {over} (bounds {NUMPY_ULP[ty]})"
