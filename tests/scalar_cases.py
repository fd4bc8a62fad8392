"""Apply bodies that evaluate one scalar op per row over every value pair of the tables in scalar_spec.py, and the
fields and admissible results that go with them.  Shared by the oracle-vs-spec CPU tests and the device-vs-spec GPU
tests, so both judge the very same module text.

A module is one nonlinear opdef @ops whose apply picks its case by the first index (a chain of scf.if on
`%i0 == row`).  Row r holds case r; its value pairs run along the remaining dimensions, the last one ending one cell
early so that one case can read an operand at offset +1 along it.  Integer cases take their operands as i64 values
assembled from two exact binary64 halves (fptosi hi + fptosi lo), narrowed with trunci / index_cast, and return
through sitofp (select for i1), so a 64-bit wrap or a low bit that sitofp rounds away is still seen."""
import itertools
import re

import numpy as np

import scalar_spec as S

NP = {S.F64: np.float64, S.F32: np.float32}
UINT = {S.F64: np.uint64, S.F32: np.uint32}


class Case:
    """name; lines(ty) -> MLIR lines ending in `%r = ...` of the apply's element type; cells: list of input tuples;
    spec(*inputs) -> Adm, or POISON (not compared)"""

    def __init__(self, name, lines, cells, spec, offset=False):
        self.name, self.lines, self.cells, self.spec, self.offset = name, lines, cells, spec, offset


def _pairs(ty):
    t = S.FLOAT_TABLE[ty]
    return [(x, y, 0.0, 0.0) for x, y in itertools.product(t, t)]


def _sel(cond, ty):
    return [f"%one = arith.constant 1.0 : {ty}", f"%zero = arith.constant 0.0 : {ty}",
            f"%r = arith.select {cond}, %one, %zero : {ty}"]


def _fadm(x, ty):
    return S.Adm([S.bits(x, ty)])


def float_cases(ty):
    """every float op, every cmpf predicate, select, and the f32 <-> f64 conversions, on the float table of `ty`"""
    cells = _pairs(ty)
    cs = []
    for op, f in S.BINARY_FLOAT.items():
        cs.append(Case(op, [f"%r = {op} %x, %y : {ty}"], cells, lambda x, y, *_, f=f: f(x, y, ty)))
    for op, f in S.UNARY_FLOAT.items():
        cs.append(Case(op, [f"%r = {op} %x : {ty}"], cells, lambda x, *_, f=f: f(x, ty)))
    for p in S.CMPF_PREDICATES:
        cs.append(Case("cmpf " + p, [f"%c = arith.cmpf {p}, %x, %y : {ty}"] + _sel("%c", ty), cells,
                       lambda x, y, *_, p=p: _fadm(1.0 if S.cmpf(p, x, y) else 0.0, ty)))
    cs.append(Case("select", [f"%c = arith.cmpf ult, %x, %y : {ty}", f"%r = arith.select %c, %y, %x : {ty}"], cells,
                   lambda x, y, *_: S.Adm([S.bits(y if S.cmpf("ult", x, y) else x, ty)])))
    # one operand read at offset +1 along the last dimension: the op runs in a tile that keeps a halo of that input
    cs.append(Case("arith.maximumf (operand at an offset)", ["%r = arith.maximumf %x, %yo : " + ty], cells,
                   lambda x, y, *_: S.maximumf(x, y, ty), offset=True))
    cs.append(Case("arith.minnumf (operand at an offset)", ["%r = arith.minnumf %yo, %x : " + ty], cells,
                   lambda x, y, *_: S.minnumf(y, x, ty), offset=True))
    if ty == S.F64:
        def f64_via_f32(x, *_):
            t = S.truncf(x)
            if t.any_nan:
                return S.ANY_NAN
            return S.extf(S.from_bits(next(iter(t.bits)), S.F32))
        cs.append(Case("truncf + extf", ["%t = arith.truncf %x : f64 to f32", "%r = arith.extf %t : f32 to f64"],
                       cells, f64_via_f32))
    else:
        cs.append(Case("extf, mulf f64, truncf",
                       ["%xe = arith.extf %x : f32 to f64", "%ye = arith.extf %y : f32 to f64",
                        "%p = arith.mulf %xe, %ye : f64", "%r = arith.truncf %p : f64 to f32"],
                       cells, lambda x, y, *_: S.truncf(x * y)))
    return cs


# ---- integer cases (f64 fields) ------------------------------------------------------------------------------------
INT_TYPES = ("i64", "i32", "i1", "index")


def _int_cells():
    out = []
    for a, b in itertools.product(S.INT_TABLE, S.INT_TABLE):
        out.append(S.split_i64(a) + S.split_i64(b))
    return out


def _operand_lines(ity):
    """%a, %b of type ity from the four f64 inputs"""
    L = ["%ah = arith.fptosi %xh : f64 to i64", "%al = arith.fptosi %xl : f64 to i64", "%a64 = arith.addi %ah, %al : i64",
         "%bh = arith.fptosi %yh : f64 to i64", "%bl = arith.fptosi %yl : f64 to i64", "%b64 = arith.addi %bh, %bl : i64"]
    if ity == "i64":
        return L + ["%a = arith.addi %a64, %zero64 : i64", "%b = arith.addi %b64, %zero64 : i64"]
    if ity == "index":
        return L + ["%a = arith.index_cast %a64 : i64 to index", "%b = arith.index_cast %b64 : i64 to index"]
    return L + [f"%a = arith.trunci %a64 : i64 to {ity}", f"%b = arith.trunci %b64 : i64 to {ity}"]


def _int_out(ity, v="%v"):
    """an ity value -> %r : f64, exactly where the integer fits in a double"""
    if ity == "i1":
        return _sel(v, "f64")
    if ity == "index":
        return [f"%v64 = arith.index_cast {v} : index to i64", "%r = arith.sitofp %v64 : i64 to f64"]
    return [f"%r = arith.sitofp {v} : {ity} to f64"]


def _int_out_spec(v, ity):
    if ity == "i1":
        return S.Adm([S.bits(1.0 if v else 0.0, S.F64)])
    return S.sitofp(S.wrap(S.signed(v, ity), "i64"), "i64", S.F64)


def _ops_in(xh, xl, yh, yl, ity):
    a = S.wrap(int(xh) + int(xl), "i64")
    b = S.wrap(int(yh) + int(yl), "i64")
    cast = S.index_cast if ity == "index" else S.trunci
    return cast(a, "i64", ity), cast(b, "i64", ity)


def int_cases():
    cells = _int_cells()
    cs = []
    for ity in INT_TYPES:
        for op, f in S.BINARY_INT.items():
            cs.append(Case(f"{op} {ity}", _operand_lines(ity) + [f"%v = {op} %a, %b : {ity}"] + _int_out(ity), cells,
                           lambda *c, f=f, ity=ity: _int_out_spec(f(*_ops_in(*c, ity), ity), ity)))
        for p in S.CMPI_PREDICATES:
            cs.append(Case(f"cmpi {p} {ity}", _operand_lines(ity) + [f"%v = arith.cmpi {p}, %a, %b : {ity}"] + _int_out("i1"),
                           cells, lambda *c, p=p, ity=ity: _int_out_spec(S.cmpi(p, *_ops_in(*c, ity), ity), "i1")))
    for ity in ("i64", "i32", "i1"):
        for fty in (S.F64, S.F32):
            for conv, f in (("sitofp", S.sitofp), ("uitofp", S.uitofp)):
                L = _operand_lines(ity) + [f"%v = arith.{conv} %a : {ity} to {fty}"]
                L += ["%r = arith.addf %v, %zerof : f64"] if fty == S.F64 else ["%r = arith.extf %v : f32 to f64"]

                def spec(*c, f=f, ity=ity, fty=fty):
                    adm = f(_ops_in(*c, ity)[0], ity, fty)
                    x = S.from_bits(next(iter(adm.bits)), fty)
                    return S.Adm([S.bits(x, S.F64)])
                cs.append(Case(f"{conv} {ity} to {fty}", L, cells, spec))
    for src, dst in (("i1", "i64"), ("i32", "i64"), ("i1", "i32")):
        L = _operand_lines(src) + [f"%v = arith.extsi %a : {src} to {dst}"] + _int_out(dst)
        cs.append(Case(f"extsi {src} to {dst}", L, cells,
                       lambda *c, src=src, dst=dst: _int_out_spec(S.extsi(_ops_in(*c, src)[0], src, dst), dst)))
    for src, dst in (("i32", "index"), ("i1", "index"), ("index", "i32")):
        L = _operand_lines(src) + [f"%v = arith.index_cast %a : {src} to {dst}"] + _int_out(dst)
        cs.append(Case(f"index_cast {src} to {dst}", L, cells,
                       lambda *c, src=src, dst=dst: _int_out_spec(S.index_cast(_ops_in(*c, src)[0], src, dst), dst)))
    # fptosi of table floats (f64, and f32 through truncf), poison outside the destination's range
    fcells = [(x, 0.0, 0.0, 0.0) for x in S.FLOAT_TABLE[S.F64]] + [(float(v), 0.0, 0.0, 0.0) for v in
                                                                   (2.0**31 - 1, -2.0**31, 2.0**31, -2.0**31 - 1, 2.0**63, -2.0**63,
                                                                    2.0**63 - 1024, 123456789.75, -0.99)]
    for fty in (S.F64, S.F32):
        for ity in ("i64", "i32"):
            pre = [] if fty == S.F64 else ["%xt = arith.truncf %xh : f64 to f32"]
            src = "%xh" if fty == S.F64 else "%xt"

            def spec(x, *_, fty=fty, ity=ity):
                if fty == S.F32:
                    t = S.truncf(x)
                    if t.any_nan:
                        return S.POISON
                    x = S.from_bits(next(iter(t.bits)), S.F32)
                v = S.fptosi(x, fty, ity)
                return S.POISON if v is S.POISON else _int_out_spec(v, ity)
            cs.append(Case(f"fptosi {fty} to {ity}", pre + [f"%v = arith.fptosi {src} : {fty} to {ity}"] + _int_out(ity),
                           fcells, spec))
    return cs


# ---- module text, fields, expected results ---------------------------------------------------------------------------
def layout(cases, rank):
    """the field shape: rows of cases; the pairs along the last dimension (2-D) or the last two (3-D), last column
    spare"""
    n = max(len(c.cells) for c in cases)
    if rank == 2:
        w = -(-(n + 1) // 64) * 64
        return (len(cases), w)
    w = -(-(-(-n // 2) + 1) // 64) * 64
    return (len(cases), 2, w)


def _coords(shape, p):
    return (p,) if len(shape) == 2 else (p // (shape[2] - 1), p % (shape[2] - 1))


def module_text(cases, ty, shape, name="ops"):
    rank = len(shape)
    ofs = lambda o: ", ".join(["0"] * (rank - 1) + [str(o)])
    lb = ", ".join(["0"] * rank)
    ub = ", ".join(str(n) for n in shape)
    bub = ", ".join([str(n) for n in shape[:-1]] + [str(shape[-1] - 1)])
    idx = ", ".join(f"%i{d}: index" for d in range(rank))
    body = [f"%x = neptune_ir.access %in0[{ofs(0)}] : !t -> {ty}", f"%y = neptune_ir.access %in1[{ofs(0)}] : !t -> {ty}",
            f"%yo = neptune_ir.access %in1[{ofs(1)}] : !t -> {ty}",
            f"%xh = neptune_ir.access %in0[{ofs(0)}] : !t -> {ty}", f"%xl = neptune_ir.access %in1[{ofs(0)}] : !t -> {ty}",
            f"%yh = neptune_ir.access %in2[{ofs(0)}] : !t -> {ty}", f"%yl = neptune_ir.access %in3[{ofs(0)}] : !t -> {ty}",
            "%zero64 = arith.constant 0 : i64", f"%zerof = arith.constant 0.0 : {ty}"]

    def chain(k, ind):
        c = cases[k]
        out = []
        if k == len(cases) - 1:
            return [ind + l for l in _rename(c.lines, k)] + [ind + f"scf.yield %r_{k} : {ty}"]
        out.append(ind + f"%k{k} = arith.constant {k} : index")
        out.append(ind + f"%q{k} = arith.cmpi eq, %i0, %k{k} : index")
        out.append(ind + f"%s{k} = scf.if %q{k} -> ({ty}) {{")
        out += [ind + "  " + l for l in _rename(c.lines, k)]
        out.append(ind + f"  scf.yield %r_{k} : {ty}")
        out.append(ind + "} else {")
        out += chain(k + 1, ind + "  ")
        out.append(ind + "}")
        out.append(ind + f"scf.yield %s{k} : {ty}")
        return out
    inner = chain(0, "")
    # the outermost level yields from the apply, not from an scf.if
    assert inner[-1].startswith("scf.yield %s0") or len(cases) == 1
    inner = inner[:-1] + [f"neptune_ir.yield %s0 : {ty}"] if len(cases) > 1 else \
        inner[:-1] + [f"neptune_ir.yield %r_0 : {ty}"]
    lines = ['#l = #neptune_ir.location<"cell">', f"#b = #neptune_ir.bounds<lb = [{lb}], ub = [{ub}]>",
             f"!t = !neptune_ir.temp<element = {ty}, bounds = #b, location = #l>", "module {",
             f"  neptune_ir.nonlinear_opdef @{name} : (!t, !t, !t, !t) -> !t {{",
             "  ^bb0(%u0: !t, %u1: !t, %u2: !t, %u3: !t):",
             "    %res = neptune_ir.apply(%u0, %u1, %u2, %u3) attributes {bounds = "
             f"#neptune_ir.bounds<lb = [{lb}], ub = [{bub}]>}} : (!t, !t, !t, !t) -> !t {{",
             f"      ^bb0({idx}, %in0: !t, %in1: !t, %in2: !t, %in3: !t):"]
    lines += ["        " + l for l in body + inner]
    lines += ["    }", "    neptune_ir.return %res : !t", "  }", "}"]
    return "\n".join(lines) + "\n"


def _rename(lines, k):
    """give each case's local values a suffix of their own (SSA names are module-unique)"""
    local = set()
    for l in lines:
        m = re.match(r"\s*(%\w+) = ", l)
        if m:
            local.add(m.group(1))
    return [re.sub(r"%\w+", lambda m: m.group(0) + f"_{k}" if m.group(0) in local else m.group(0), l) for l in lines]


def fields(cases, ty, shape):
    """the four input fields, and per case row the admissible results (None = not compared) at each pair's cell"""
    dt = NP[ty]
    ins = [np.ones(shape, dtype=dt) for _ in range(4)]
    expect = {}
    for r, c in enumerate(cases):
        for p in range(len(c.cells)):
            at = (r,) + _coords(shape, p)
            cell = c.cells[p]
            for k in range(4):
                if c.offset and k == 1:         # operand 1 is read at +1 along the last dimension
                    ins[1][at[:-1] + (at[-1] + 1,)] = cell[1]
                else:
                    ins[k][at] = cell[k]
    for r, c in enumerate(cases):   # the spec sees the values as stored (binary32 inputs rounded)
        for p in range(len(c.cells)):
            at = (r,) + _coords(shape, p)
            cell = [float(ins[k][at]) for k in range(4)]
            if c.offset:
                cell[1] = float(ins[1][at[:-1] + (at[-1] + 1,)])
            expect[at] = c.spec(*cell)
    return ins, expect


def check(got, expect, cases, ty, what=""):
    """every compared cell admitted by the spec (NaN where the spec says NaN, else bit for bit); returns the number
    of cells compared and a report of the first mismatches per case"""
    u = got.view(UINT[ty])
    bad = {}
    n = 0
    for at, adm in expect.items():
        if adm is S.POISON:
            continue
        n += 1
        b = int(u[at])
        if not adm.admits(b, ty):
            bad.setdefault(cases[at[0]].name, []).append((at, S.from_bits(b, ty), adm))
    lines = []
    for name, l in bad.items():
        lines.append(f"{what}{name}: {len(l)} cells, e.g. " + "; ".join(f"{at} got {g!r} want {a}" for at, g, a in l[:3]))
    return n, "\n".join(lines)

# ---- elementary functions against a 120-bit reference ------------------------------------------------------------------
ELEMENTARY = ("math.exp", "math.log", "math.sin", "math.cos", "math.tanh", "math.powf")


def _grid(ty):
    """dense argument grids per function: the finite-result domain, subnormal and near-overflow results, log near 1,
    sin / cos near multiples of pi/2 and far out, tanh of tiny arguments, pow of negative bases at integer exponents"""
    rng = np.random.default_rng(1234 if ty == S.F64 else 4321)
    f64 = ty == S.F64
    big, lo_e, hi_e = (709.78, -745.1, 709.78) if f64 else (88.72, -103.9, 88.72)
    tiny_e = -300 if f64 else -44
    g = {}
    g["math.exp"] = [(x, 1.0) for x in np.concatenate([np.linspace(lo_e, hi_e, 1500), np.linspace(lo_e, lo_e + 40, 300),
                                                       np.linspace(hi_e - 10, hi_e, 200), rng.uniform(-1, 1, 200),
                                                       np.logspace(tiny_e, -1, 100), -np.logspace(tiny_e, -1, 100)])]
    eps = 2.0**-52 if f64 else 2.0**-23
    near1 = 1 + np.arange(-300, 301) * eps * 7
    g["math.log"] = [(x, 1.0) for x in np.concatenate([np.logspace(-307 if f64 else -37, 308 if f64 else 38, 1200),
                                                       [5e-324 if f64 else 1.4e-45, 1e-310 if f64 else 1e-40],
                                                       near1, np.linspace(0.5, 2, 300)])]
    half_pi = np.arange(-400, 401) * (np.pi / 2)          # k pi/2, and a few ulps either side of it
    near = half_pi[:, None] + np.array([-2, -1, 0, 1, 2]) * eps * np.maximum(1, np.abs(half_pi))[:, None]
    huge = [1e22, -1e22, 1e300, 2.0**1000, 1.7976931348623157e308] if f64 else [1e22, 1e30, -3e38, 3.4e38]
    sc = np.concatenate([np.linspace(-10, 10, 800), near.ravel(), rng.uniform(-1e5, 1e5, 800), huge])
    g["math.sin"] = [(x, 1.0) for x in sc]
    g["math.cos"] = [(x, 1.0) for x in sc]
    g["math.tanh"] = [(x, 1.0) for x in np.concatenate([np.linspace(-20, 20, 1000), np.logspace(tiny_e, -1, 300),
                                                        -np.logspace(tiny_e, -1, 300)])]
    pw = [(x, y) for x, y in zip(rng.uniform(0.1, 10, 800), rng.uniform(-30, 30, 800))]
    pw += [(x, float(y)) for x, y in zip(rng.uniform(-10, -0.1, 600), rng.integers(-20, 21, 600))]
    pw += [(2.0, y) for y in np.linspace(1000, 1023.99, 100)] if f64 else [(2.0, y) for y in np.linspace(100, 127.99, 100)]
    pw += [(0.5, y) for y in np.linspace(1000, 1074, 100)] if f64 else [(0.5, y) for y in np.linspace(120, 149, 100)]
    g["math.powf"] = pw
    dt = NP[ty]
    return {f: [(float(dt(x)), float(dt(y)), 0.0, 0.0) for x, y in v] for f, v in g.items()}


def _nan():
    return float("nan")


_INF = float("inf")


def special_values():
    """C99 Annex F special cases: (function, x, y, exact result); NaN means any NaN"""
    nan, inf = _nan(), _INF
    t = [("math.exp", inf, 0, inf), ("math.exp", -inf, 0, 0.0), ("math.exp", 0.0, 0, 1.0), ("math.exp", -0.0, 0, 1.0),
         ("math.exp", nan, 0, nan), ("math.exp", 1e4, 0, inf), ("math.exp", -1e4, 0, 0.0),
         ("math.log", 0.0, 0, -inf), ("math.log", -0.0, 0, -inf), ("math.log", 1.0, 0, 0.0), ("math.log", -1.0, 0, nan),
         ("math.log", -inf, 0, nan), ("math.log", inf, 0, inf), ("math.log", nan, 0, nan),
         ("math.sin", 0.0, 0, 0.0), ("math.sin", -0.0, 0, -0.0), ("math.sin", inf, 0, nan), ("math.sin", -inf, 0, nan),
         ("math.cos", 0.0, 0, 1.0), ("math.cos", -0.0, 0, 1.0), ("math.cos", inf, 0, nan), ("math.cos", -inf, 0, nan),
         ("math.tanh", 0.0, 0, 0.0), ("math.tanh", -0.0, 0, -0.0), ("math.tanh", inf, 0, 1.0), ("math.tanh", -inf, 0, -1.0),
         ("math.tanh", nan, 0, nan)]
    P = []
    for x in (nan, -inf, -2.0, -0.0, 0.0, 0.5, 3.0, inf):
        P += [(x, 0.0, 1.0), (x, -0.0, 1.0)]                     # pow(x, +-0) = 1 for any x
    for y in (nan, -inf, -3.0, 0.5, inf):
        P.append((1.0, y, 1.0))                                  # pow(+1, y) = 1 for any y
    P += [(0.0, -3.0, inf), (-0.0, -3.0, -inf), (0.0, -2.0, inf), (-0.0, -2.0, inf), (-0.0, -0.5, inf),
          (0.0, -inf, inf), (-0.0, -inf, inf), (0.0, 3.0, 0.0), (-0.0, 3.0, -0.0), (-0.0, 2.0, 0.0), (-0.0, 0.5, 0.0),
          (-1.0, inf, 1.0), (-1.0, -inf, 1.0), (0.5, -inf, inf), (-0.5, -inf, inf), (2.0, -inf, 0.0), (-2.0, -inf, 0.0),
          (0.5, inf, 0.0), (-0.5, inf, 0.0), (2.0, inf, inf), (-2.0, inf, inf),
          (-inf, -3.0, -0.0), (-inf, -2.0, 0.0), (-inf, -0.5, 0.0), (-inf, 3.0, -inf), (-inf, 2.0, inf), (-inf, 0.5, inf),
          (inf, -2.0, 0.0), (inf, 0.5, inf), (-2.0, 0.5, nan), (-2.0, 3.0, -8.0), (-2.0, -3.0, -0.125), (-3.0, 2.0, 9.0),
          (nan, 1.0, nan), (2.0, nan, nan)]
    t += [("math.powf", x, y, r) for x, y, r in P]
    return t


def elementary_cases(ty):
    g = _grid(ty)
    cs = []
    for f in ELEMENTARY:
        line = f"%r = {f} %x, %y : {ty}" if f == "math.powf" else f"%r = {f} %x : {ty}"
        cells = g[f] + [(x, float(y), 0.0, 0.0) for ff, x, y, _ in special_values() if ff == f]
        cs.append(Case(f, [line], cells, None))
    return cs


def special_adm(f, x, y, ty):
    """the exact result where Annex F fixes it, else None"""
    for ff, sx, sy, r in special_values():
        if ff == f and S.bits(sx, S.F64) == S.bits(x, S.F64) and (f != "math.powf" or S.bits(float(sy), S.F64) == S.bits(y, S.F64)):
            return S.ANY_NAN if r != r else S.Adm([S.bits(r, ty)])
    return None


_REF = {}


def reference(f, x, y, ty):
    """(correctly rounded result, its ulp, the 120-bit value) or None where the result is not finite and nonzero
    in `ty`"""
    key = (f, x, y, ty)
    if key in _REF:
        return _REF[key]
    import mpmath
    with mpmath.workprec(120):
        X = mpmath.mpf(x)
        try:
            if f == "math.exp":
                v = mpmath.exp(X)
            elif f == "math.log":
                v = mpmath.log(X) if x > 0 else None
            elif f == "math.sin":
                v = mpmath.sin(X)
            elif f == "math.cos":
                v = mpmath.cos(X)
            elif f == "math.tanh":
                v = mpmath.tanh(X)
            else:
                Y = mpmath.mpf(y)
                v = mpmath.power(X, Y) if (x > 0 or float(y).is_integer()) and x != 0 else None
        except (ValueError, ZeroDivisionError):
            v = None
        out = None
        if v is not None and mpmath.isfinite(v) and v != 0 and not isinstance(v, mpmath.mpc):
            r = S.rnd(float(v), ty)
            if r == r and abs(r) != _INF and r != 0:
                p, emin = (53, -1022) if ty == S.F64 else (24, -126)
                e = max(mpmath.floor(mpmath.log(abs(mpmath.mpf(r)), 2)), emin)
                out = (r, mpmath.mpf(2) ** (e - p + 1), v)
    _REF[key] = out
    return out


def ulp_error(got, ref):
    import mpmath
    r, ulp, v = ref
    if got != got or abs(got) == _INF:
        return float("inf")
    with mpmath.workprec(120):
        return float(abs(mpmath.mpf(got) - v) / ulp)


def elementary_check(got, cases, ty, shape):
    """per function: the largest ulp error over the grid, and the special values that are off"""
    worst, bad = {}, []
    u = got.view(UINT[ty])
    for r, c in enumerate(cases):
        w = 0.0
        for p, cell in enumerate(c.cells):
            at = (r,) + _coords(shape, p)
            x, y = cell[0], cell[1]
            g = float(got[at])
            sp = special_adm(c.name, x, y, ty)
            if sp is not None:
                if not sp.admits(int(u[at]), ty):
                    bad.append(f"{c.name}({x!r}, {y!r}) = {g!r}, want {sp}")
                continue
            ref = reference(c.name, x, y, ty)
            if ref is None:
                continue
            w = max(w, ulp_error(g, ref))
        worst[c.name] = w
    return worst, bad


def elementary_fields(cases, ty, shape):
    dt = NP[ty]
    ins = [np.ones(shape, dtype=dt) for _ in range(4)]
    for r, c in enumerate(cases):
        for p, cell in enumerate(c.cells):
            at = (r,) + _coords(shape, p)
            ins[0][at], ins[1][at] = cell[0], cell[1]
    return ins
