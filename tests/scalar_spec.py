"""An independent model of the scalar ops an apply body may contain (csrc/lowering/verify.cpp, check_arith), written
from the MLIR arith / math definitions and, where MLIR defers to it, LLVM LangRef -- the reference lowers these ops
through arith-to-llvm and math-to-llvm, so those documents are the specification.

Plain Python only: no numpy ufuncs, no oracle.  Floats are Python floats (binary64); a binary32 result is the binary64
result rounded once more with struct.pack('f', ...).  For + - * / and sqrt of binary32 operands that double rounding
is innocuous (binary64 has more than 2*24+2 bits), so it gives the correctly rounded binary32 result; integer ->
binary32 conversions are rounded from the exact integer instead (int_to_float).

Integers are bit patterns: a value of type iN is an int in [0, 2**N); `signed()` reads it as two's complement.
`index` is 64 bits wide (the reference's target).  i1 true is the pattern 1, whose signed value is -1.

Every function returns the admissible results as an `Adm`:
  * usually one bit pattern;
  * ANY_NAN for a NaN the op generates or propagates (LLVM leaves its payload and sign open);
  * exact bits where the op is a bit operation even on NaN: negf, absf, copysign (IEEE 754 5.5.1);
  * both zeros for maxnumf / minnumf of (+0, -0) in either order (MLIR / llvm.maxnum leave the choice open).
Integer and i1 results are plain ints (patterns); a comparison returns a bool.

Poison: `fptosi` of NaN, of an infinity or of a value whose truncation does not fit the destination is poison in
MLIR (LangRef fptosi).  Such cases return POISON and are not compared.
"""
import math
import struct

F32, F64 = "f32", "f64"
FLOATS = (F32, F64)
WIDTH = {"i1": 1, "i32": 32, "i64": 64, "index": 64}
POISON = None


class Adm:
    """the set of admissible bit patterns of one float result"""
    __slots__ = ("bits", "any_nan")

    def __init__(self, bits=(), any_nan=False):
        self.bits = frozenset(bits)
        self.any_nan = any_nan

    def admits(self, b: int, ty: str) -> bool:
        if self.any_nan and is_nan_bits(b, ty):
            return True
        return b in self.bits

    def __repr__(self):
        if self.any_nan:
            return "Adm(any NaN)"
        return "Adm(" + ", ".join(hex(b) for b in sorted(self.bits)) + ")"


ANY_NAN = Adm(any_nan=True)


# ---- bit patterns ------------------------------------------------------------------------------------------------
def bits(x: float, ty: str) -> int:
    if ty == F64:
        return struct.unpack("<Q", struct.pack("<d", x))[0]
    return struct.unpack("<I", struct.pack("<f", x))[0]


def from_bits(b: int, ty: str) -> float:
    if ty == F64:
        return struct.unpack("<d", struct.pack("<Q", b))[0]
    return struct.unpack("<f", struct.pack("<I", b))[0]


def sign_mask(ty: str) -> int:
    return 1 << 63 if ty == F64 else 1 << 31


def is_nan_bits(b: int, ty: str) -> bool:
    if ty == F64:
        return (b & 0x7FF0000000000000) == 0x7FF0000000000000 and (b & 0x000FFFFFFFFFFFFF) != 0
    return (b & 0x7F800000) == 0x7F800000 and (b & 0x007FFFFF) != 0


def rnd(x: float, ty: str) -> float:
    """round a binary64 value to `ty` (round to nearest, ties to even; overflow to infinity)"""
    if ty == F64 or x != x or math.isinf(x):
        return x
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:             # struct refuses exactly when the rounded value is infinite
        return math.copysign(math.inf, x)


def one(x: float, ty: str) -> Adm:
    """the admissible set of a rounded arithmetic result: its bits, or any NaN"""
    x = rnd(x, ty)
    return ANY_NAN if x != x else Adm([bits(x, ty)])


def is_nan(x: float) -> bool:
    return x != x


# ---- floating-point arithmetic -----------------------------------------------------------------------------------
def _div(a: float, b: float) -> float:
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -math.inf if neg else math.inf
    return a / b


def addf(a, b, ty): return one(a + b, ty)
def subf(a, b, ty): return one(a - b, ty)
def mulf(a, b, ty): return one(a * b, ty)
def divf(a, b, ty): return one(_div(a, b), ty)


def negf(a, ty):
    return Adm([bits(a, ty) ^ sign_mask(ty)])


def absf(a, ty):
    return Adm([bits(a, ty) & ~sign_mask(ty)])


def copysign(a, b, ty):
    m = sign_mask(ty)
    return Adm([(bits(a, ty) & ~m) | (bits(b, ty) & m)])


def sqrt(a, ty):
    if a != a or a < 0:
        return ANY_NAN
    return one(math.sqrt(a), ty)          # correctly rounded (IEEE), sqrt(-0) = -0, sqrt(inf) = inf


def floor(a, ty):
    if a != a:
        return ANY_NAN
    if a == 0 or math.isinf(a):
        return Adm([bits(a, ty)])
    r = float(math.floor(a))
    return Adm([bits(r, ty)])             # |a| >= 1 or a in (0, 1): no signed-zero question except below


def ceil(a, ty):
    if a != a:
        return ANY_NAN
    if a == 0 or math.isinf(a):
        return Adm([bits(a, ty)])
    r = float(math.ceil(a))
    if r == 0:
        r = -0.0                          # ceil(x) for x in (-1, 0) is -0
    return Adm([bits(r, ty)])


def _tie_zero(a, b):
    return a == 0 and b == 0


def maximumf(a, b, ty):
    """llvm.maximum: NaN if either operand is NaN; -0 < +0"""
    if a != a or b != b:
        return ANY_NAN
    if _tie_zero(a, b):
        return Adm([bits(a if math.copysign(1.0, a) > 0 else b, ty)])
    return Adm([bits(a if a > b else b, ty)])


def minimumf(a, b, ty):
    if a != a or b != b:
        return ANY_NAN
    if _tie_zero(a, b):
        return Adm([bits(a if math.copysign(1.0, a) < 0 else b, ty)])
    return Adm([bits(a if a < b else b, ty)])


def maxnumf(a, b, ty):
    """llvm.maxnum: the other operand if exactly one is NaN; either zero on a (+0, -0) tie"""
    if a != a and b != b:
        return ANY_NAN
    if a != a:
        return Adm([bits(b, ty)])
    if b != b:
        return Adm([bits(a, ty)])
    if _tie_zero(a, b):
        return Adm([bits(a, ty), bits(b, ty)])
    return Adm([bits(a if a > b else b, ty)])


def minnumf(a, b, ty):
    if a != a and b != b:
        return ANY_NAN
    if a != a:
        return Adm([bits(b, ty)])
    if b != b:
        return Adm([bits(a, ty)])
    if _tie_zero(a, b):
        return Adm([bits(a, ty), bits(b, ty)])
    return Adm([bits(a if a < b else b, ty)])


BINARY_FLOAT = {"arith.addf": addf, "arith.subf": subf, "arith.mulf": mulf, "arith.divf": divf,
                "arith.maximumf": maximumf, "arith.minimumf": minimumf, "arith.maxnumf": maxnumf,
                "arith.minnumf": minnumf, "math.copysign": copysign}
UNARY_FLOAT = {"arith.negf": negf, "math.absf": absf, "math.sqrt": sqrt, "math.floor": floor, "math.ceil": ceil}


# ---- comparisons and select --------------------------------------------------------------------------------------
CMPF_PREDICATES = ("oeq", "ogt", "oge", "olt", "ole", "one", "ord", "ueq", "ugt", "uge", "ult", "ule", "une", "uno")
CMPI_PREDICATES = ("eq", "ne", "slt", "sle", "sgt", "sge", "ult", "ule", "ugt", "uge")


def cmpf(pred: str, a: float, b: float) -> bool:
    uno = a != a or b != b
    rel = {"eq": a == b, "gt": a > b, "ge": a >= b, "lt": a < b, "le": a <= b, "ne": a != b}
    if pred == "ord":
        return not uno
    if pred == "uno":
        return uno
    if pred[0] == "o":
        return (not uno) and rel[pred[1:]]
    return uno or rel[pred[1:]]


def signed(v: int, ity: str) -> int:
    w = WIDTH[ity]
    return v - (1 << w) if v >> (w - 1) & 1 else v


def wrap(v: int, ity: str) -> int:
    return v & ((1 << WIDTH[ity]) - 1)


def cmpi(pred: str, a: int, b: int, ity: str) -> bool:
    if pred == "eq":
        return a == b
    if pred == "ne":
        return a != b
    if pred[0] == "s":
        a, b = signed(a, ity), signed(b, ity)
    return {"lt": a < b, "le": a <= b, "gt": a > b, "ge": a >= b}[pred[1:]]


def select(c: bool, a, b):
    return a if c else b


# ---- integer arithmetic (wraps: MLIR addi/subi/muli without overflow flags) --------------------------------------
def addi(a, b, ity): return wrap(a + b, ity)
def subi(a, b, ity): return wrap(a - b, ity)
def muli(a, b, ity): return wrap(a * b, ity)
def andi(a, b, ity): return a & b
def ori(a, b, ity): return a | b
def xori(a, b, ity): return a ^ b


BINARY_INT = {"arith.addi": addi, "arith.subi": subi, "arith.muli": muli, "arith.andi": andi, "arith.ori": ori,
              "arith.xori": xori}


# ---- conversions -------------------------------------------------------------------------------------------------
def int_to_float(n: int, ty: str) -> float:
    """exact integer -> nearest `ty` (ties to even), one rounding"""
    if ty == F64 or n == 0:
        return float(n)                   # int.__float__ is correctly rounded
    m, s = abs(n), (-1.0 if n < 0 else 1.0)
    e = m.bit_length()
    if e > 24:
        sh = e - 24
        q, r = m >> sh, m & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if r > half or (r == half and q & 1):
            q += 1
        m = q << sh
    return s * float(m)                   # < 2**65: finite in binary32


def sitofp(a: int, ity: str, ty: str) -> Adm:
    return Adm([bits(int_to_float(signed(a, ity), ty), ty)])


def uitofp(a: int, ity: str, ty: str) -> Adm:
    return Adm([bits(int_to_float(a, ty), ty)])


def fptosi(x: float, ty: str, ity: str):
    """truncation toward zero; POISON for NaN, infinities and out-of-range values"""
    if x != x or math.isinf(x):
        return POISON
    t = int(x)
    w = WIDTH[ity]
    if not -(1 << (w - 1)) <= t < (1 << (w - 1)):
        return POISON
    return wrap(t, ity)


def extf(x: float) -> Adm:
    """f32 -> f64: exact"""
    return ANY_NAN if x != x else Adm([bits(x, F64)])


def truncf(x: float) -> Adm:
    """f64 -> f32: round to nearest even, overflow to infinity"""
    return one(x, F32)


def extsi(a: int, ifrom: str, ito: str) -> int:
    return wrap(signed(a, ifrom), ito)


def trunci(a: int, ifrom: str, ito: str) -> int:
    return wrap(a, ito)


def index_cast(a: int, ifrom: str, ito: str) -> int:
    """sign-extends when widening, truncates when narrowing (MLIR arith.index_cast)"""
    return wrap(signed(a, ifrom), ito)


# ---- value tables ------------------------------------------------------------------------------------------------
def _f(h: str) -> float:
    return float.fromhex(h)


_NAN_POS = from_bits(0x7FF8000000000000, F64)
_NAN_NEG = from_bits(0xFFF8000000000000, F64)


def _pm(*xs):
    out = []
    for x in xs:
        out += [x, -x]
    return out


FLOAT_TABLE = {
    F64: _pm(0.0, 5e-324, _f("0x0.fffffffffffffp-1022"), _f("0x1p-1022"), 1.0, 0.5, 1.5, 2.5,
             _f("0x1.fffffffffffffp+1023"), math.inf)
    + [_f("0x1.0000000000001p+0"), _f("0x1.fffffffffffffp-1"), 3.0, -7.25, 1e10,
       _f("0x1.000001p+0"), _f("0x1.000003p+0"),        # f64 -> f32 ties: to even below, to even above
       _f("0x1.ffffffp+127"), 1e39,                      # f64 -> f32: the tie above FLT_MAX, and past it: infinity
       _f("0x1p-150"), _f("0x1.8p-149"),                 # f64 -> f32 ties in the subnormal range
       _NAN_POS, _NAN_NEG],
    F32: _pm(0.0, _f("0x1p-149"), _f("0x1.fffffcp-127"), _f("0x1p-126"), 1.0, 0.5, 1.5, 2.5,
             _f("0x1.fffffep+127"), math.inf)
    + [_f("0x1.000002p+0"), _f("0x1.fffffep-1"), 3.0, -7.25, 1e10, _f("0x1p+64"), _f("-0x1p+31"),
       _NAN_POS, _NAN_NEG],
}

# i64 values (signed); narrower types see their truncation
INT_TABLE = [0, 1, -1, 2, -2, 7, 2**31 - 1, -2**31, 2**31, 2**32 - 1, 2**24 + 1, 2**24 + 3,
             2**53 + 1, -(2**53 + 1), 2**60 + 2**36, 2**60 + 3 * 2**36, 2**62 + 1,
             2**63 - 1, -2**63, 2**63 - 1025, -2**63 + 1]


def split_i64(v: int):
    """v = hi + lo with both halves exact in binary64 and in range for fptosi to i64 (lo in [0, 2048))"""
    lo = v & 0x7FF
    hi = v - lo
    assert float(hi) == hi and -2**63 <= hi < 2**63
    return float(hi), float(lo)
