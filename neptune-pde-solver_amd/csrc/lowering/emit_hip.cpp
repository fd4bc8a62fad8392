// emit_hip.cpp -- the `backend = hip` dataflow lowering: NeptuneIR module -> one HIP translation
// unit whose host side calls the hand-written stencil kernels.
//
// It takes the place of the reference's NeptuneIRDataflowLoweringPass
// (lib/Passes/DataflowLowering.cpp:739-819, the `backend == gpu` slot at :803-804 that was never
// wired, lib/Pipeline/NeptuneIRPassesPipeline.cpp:22-26) together with the part of
// StructureLowering (lib/Passes/StructureLowering.cpp:30-124) it depends on:
//
//   linear_opdef / nonlinear_opdef @A      -> exported extern "C" symbol A + internal A__impl
//   apply_linear / apply_nonlinear @A(x)   -> call of A__impl (device-resident, no staging)
//   wrap / unwrap / load                   -> aliases                      (:131-159)
//   apply                                  -> Body functor (one C++ statement per region op, in
//                                             textual order) + run_apply<Body,...>: ONE kernel that
//                                             also does the copy-through of input 0 (:258-448)
//   store                                  -> elided when the producing apply can write straight
//                                             into the destination field, else a device copy (:165-220)
//   reduce {kind = "sum"}                  -> fixed-tree device sum (:589-698); of a single-use apply
//                                             result: ONE kernel that evaluates the body and sums
//   time_advance {method = 0, rhs = @A}    -> u + dt*A(u): one kernel when @A is a single apply of
//                                             the state, else call + axpy apply
//                                             (lib/Passes/HighLevelConvertion.cpp:77-120)
//   func.func @entry                       -> exported symbol with expanded memref arguments and a
//                                             memref struct result (upstream func-to-llvm ABI,
//                                             NeptuneIRPassesPipeline.cpp:36-40)
//
// The arithmetic inside a Body is emitted as written: no reassociation, no contraction (the TU is
// compiled with -ffp-contract=off), constants as hexadecimal floating literals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <algorithm>
#include <sstream>

#include "lowering.h"

namespace neptune_lowering {
namespace {

std::string cname(const std::string& ssa) {  // %lap_i -> v_lap_i
  std::string s = "v_";
  for (size_t i = 1; i < ssa.size(); ++i) s += (std::isalnum((unsigned char)ssa[i]) ? ssa[i] : '_');
  return s;
}
std::string ctype(const std::string& elem) {
  if (elem == "f64") return "double";
  if (elem == "f32") return "float";
  if (elem == "index" || elem == "i64") return "int64_t";
  if (elem == "i32") return "int32_t";
  if (elem == "i1") return "bool";
  return "void";
}
// the unsigned type integer arithmetic of `elem` is done in (MLIR addi / subi / muli wrap; signed C overflow would be
// undefined), and that unsigned-compares / uitofp read the source's bits through
std::string utype(const std::string& elem) { return (elem == "index" || elem == "i64") ? "uint64_t" : "uint32_t"; }
// the value of an integer operand sign-extended to 64 bits: i1 `true` is -1 (a one-bit two's complement integer)
std::string sext(const std::string& v, const std::string& elem) {
  return elem == "i1" ? "(-(int64_t)" + v + ")" : "(int64_t)" + v;
}
int esize(const std::string& elem) { return elem == "f32" ? 4 : 8; }
std::string dtype_macro(const std::string& elem) { return elem == "f32" ? "NEPTUNE_HIP_F32" : "NEPTUNE_HIP_F64"; }

std::string float_literal(const std::string& lit, const std::string& elem, bool& ok) {
  ok = true;
  char buf[64];
  if (lit.size() > 2 && (lit.compare(0, 2, "0x") == 0 || lit.compare(0, 3, "-0x") == 0)) {
    // MLIR prints infinities, NaNs and -0.0 as the bit pattern in hex, one digit per nibble of the type
    const size_t digits = elem == "f32" ? 8 : 16;
    if (lit[0] != '0' || lit.size() != 2 + digits ||
        lit.find_first_not_of("0123456789abcdefABCDEF", 2) != std::string::npos) { ok = false; return ""; }
    snprintf(buf, sizeof(buf), "__builtin_bit_cast(%s, (%s)0x%sull)", elem == "f32" ? "float" : "double",
             elem == "f32" ? "uint32_t" : "uint64_t", lit.c_str() + 2);
    return buf;
  }
  const double d = std::strtod(lit.c_str(), nullptr);
  if (elem == "f32") {
    const float f = (float)d;  // MLIR parses the literal as a double and rounds it to f32
    if (std::isinf(f) || std::isnan(f)) { ok = false; return ""; }
    snprintf(buf, sizeof(buf), "%af", (double)f);
  } else {
    if (std::isinf(d) || std::isnan(d)) { ok = false; return ""; }
    snprintf(buf, sizeof(buf), "%a", d);
  }
  return buf;
}

std::string box_init(const Bounds& b) {
  std::ostringstream o;
  o << "{" << b.rank() << ", {";
  for (int d = 0; d < 6; ++d) o << (d ? ", " : "") << (d < b.rank() ? b.lb[d] : 0);
  o << "}, {";
  for (int d = 0; d < 6; ++d) o << (d ? ", " : "") << (d < b.rank() ? b.ub[d] : 1);
  o << "}}";
  return o.str();
}

struct Footprint {
  int nin = 0, rank = 0;
  int radius[4][3];      // all accesses
  int top_radius[4][3];  // unconditional accesses only; -1 = none
  int top_lo[4][3], top_hi[4][3];  // ... as offsets: most negative / most positive; hi < lo = none
  bool box = false;
  int halo_input = -1;
  unsigned halo_mask = 0;
  int halo_inputs = 0;
  int R[3] = {0, 0, 0};  // shared radii on the kernel's (I,J,K) axes
  bool march_ok = true;
  int lead = 0;          // leading (batch / component) dimensions of an apply of rank 4..6: peeled off on the host
  // rank 4..6 with offsets along a leading dimension: a stencil in more than three dimensions, run by the rank-generic
  // kernel (kernels/apply_nd.hpp) -- what its unconditional accesses reach per input and dimension, its reach along dim 0
  bool nd = false;
  int nd_lo[4][6], nd_hi[4][6];
  int nd_halo0 = 0;
  bool exact = true;     // no elementary functions in the body
};

struct Emitter {
  const Module& m;
  Diag& diag;
  LowerInfo& info;
  std::ostringstream bodies, funcs, geom_entries;
  bool saw_elementary = false;  // set by emit_op when it emits exp/log/sin/cos/tanh/powf
  bool nd_body = false;         // emitting the body of a Footprint::nd apply: accesses carry one offset per dimension
  int box_counter = 0;
  std::ostringstream consts;
  Emitter(const Module& mm, Diag& d, LowerInfo& i) : m(mm), diag(d), info(i) {}

  std::string new_box(const Bounds& b) {
    std::string name = "kBox" + std::to_string(box_counter++);
    consts << "static const nl::Box " << name << " = " << box_init(b) << ";\n";
    return name;
  }

  // ---- apply region -> Body functor ----------------------------------------------------
  void scan_accesses(const Block& blk, const std::map<std::string, int>& temp_index, Footprint& fp, bool top) {
    for (auto& op : blk.ops) {
      if (op->name == "neptune_ir.access") {
        const int k = temp_index.at(op->operands[0]);
        int nz = 0;
        for (int d = 0; d < fp.rank; ++d) {
          const int a = (int)std::llabs(op->offsets[fp.lead + d]);
          if (a) ++nz;
          if (a > fp.radius[k][d]) fp.radius[k][d] = a;
          if (top && a > fp.top_radius[k][d]) fp.top_radius[k][d] = a;  // starts at -1: offset 0 counts
          if (top) {
            const int off = (int)op->offsets[fp.lead + d];
            if (fp.top_hi[k][d] < fp.top_lo[k][d]) fp.top_lo[k][d] = fp.top_hi[k][d] = off;   // the first unconditional access
            else { fp.top_lo[k][d] = std::min(fp.top_lo[k][d], off); fp.top_hi[k][d] = std::max(fp.top_hi[k][d], off); }
          }
        }
        if (nz > 1) fp.box = true;
      }
      for (auto& r : op->regions) scan_accesses(*r, temp_index, fp, false);
    }
  }

  bool emit_region_ops(const Block& blk, std::ostringstream& o, const std::string& ind,
                       const std::map<std::string, int>& temp_index, const std::map<std::string, int>& index_arg,
                       const std::vector<std::string>* if_results) {
    for (auto& opp : blk.ops)
      if (!emit_op(*opp, o, ind, temp_index, index_arg, if_results)) return false;
    return true;
  }

  // one scalar op -> one C++ statement (also used for scalar arithmetic at function level, where
  // the same text is valid host code)
  bool emit_op(const Op& op, std::ostringstream& o, const std::string& ind, const std::map<std::string, int>& temp_index,
               const std::map<std::string, int>& index_arg, const std::vector<std::string>* if_results) {
    {
      const std::string& n = op.name;
      auto val = [&](const std::string& v) -> std::string {
        auto it = index_arg.find(v);
        if (it != index_arg.end())
          return it->second < 0 ? "lead[" + std::to_string(-it->second - 1) + "]" : "a.template idx<" + std::to_string(it->second) + ">()";
        return cname(v);
      };
      auto res = [&]() { return cname(op.results.at(0)); };
      if (n == "neptune_ir.access") {
        o << ind << "const " << ctype(op.types[1].elem) << " " << res() << " = a.template get<" << temp_index.at(op.operands[0]);
        for (size_t d = (op.offsets.size() > 3 && !nd_body) ? op.offsets.size() - 3 : 0; d < op.offsets.size(); ++d) o << ", " << op.offsets[d];
        o << ">();\n";
      } else if (n == "arith.constant") {
        const Type& t = op.types[0];
        if (t.elem == "f64" || t.elem == "f32") {
          bool ok;
          std::string lit = float_literal(op.literal, t.elem, ok);
          if (!ok) {
            const bool hex = op.literal.find("0x") != std::string::npos;
            diag.fail(op.line, "unsupported floating-point constant '" + op.literal + "'" +
                                   (hex ? std::string(" (a hex constant is the bit pattern: 0x and exactly ") +
                                              (t.elem == "f32" ? "8" : "16") + " hex digits for " + t.elem + ")"
                                        : std::string()));
            return false;
          }
          o << ind << "const " << ctype(t.elem) << " " << res() << " = " << lit << ";  // " << op.literal << "\n";
        } else if (t.elem == "i1") {
          o << ind << "const bool " << res() << " = " << ((op.literal == "true" || op.literal == "1") ? "true" : "false") << ";\n";
        } else {
          o << ind << "const " << ctype(t.elem) << " " << res() << " = (" << ctype(t.elem) << ")" << op.literal << "LL;\n";
        }
      } else if (n == "arith.addf" || n == "arith.subf" || n == "arith.mulf" || n == "arith.divf") {
        const char* sym = (n.find("add") != std::string::npos) ? "+" : (n.find("sub") != std::string::npos) ? "-"
                          : (n.find("mul") != std::string::npos) ? "*" : "/";
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = " << val(op.operands[0]) << " " << sym << " "
          << val(op.operands[1]) << ";\n";
      } else if (n == "arith.addi" || n == "arith.subi" || n == "arith.muli") {
        // wrapping integer arithmetic: in the unsigned type of the width, then back (i1: the low bit)
        const std::string& e = op.types[0].elem;
        const std::string u = utype(e);
        const char* sym = n == "arith.addi" ? "+" : n == "arith.subi" ? "-" : "*";
        const std::string x = "(" + u + ")" + val(op.operands[0]) + " " + sym + " (" + u + ")" + val(op.operands[1]);
        o << ind << "const " << ctype(e) << " " << res() << " = "
          << (e == "i1" ? "((" + x + ") & 1u) != 0" : "(" + ctype(e) + ")(" + u + ")(" + x + ")") << ";\n";
      } else if (n == "arith.andi" || n == "arith.ori" || n == "arith.xori") {
        const bool b1 = op.types[0].elem == "i1";
        const char* sym = n == "arith.andi" ? (b1 ? "&&" : "&") : n == "arith.ori" ? (b1 ? "||" : "|") : (b1 ? "!=" : "^");
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = " << val(op.operands[0]) << " " << sym << " "
          << val(op.operands[1]) << ";\n";
      } else if (n == "arith.negf") {
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = -" << val(op.operands[0]) << ";\n";
      } else if (n == "arith.maximumf" || n == "arith.minimumf" || n == "arith.maxnumf" || n == "arith.minnumf") {
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = neptune_hip::ops::" << n.substr(6) << "("
          << val(op.operands[0]) << ", " << val(op.operands[1]) << ");\n";
      } else if (n == "math.copysign") {
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = neptune_hip::ops::copysign(" << val(op.operands[0])
          << ", " << val(op.operands[1]) << ");\n";
      } else if (n == "math.powf") {
        saw_elementary = true;
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = neptune_hip::ops::powf(" << val(op.operands[0]) << ", "
          << val(op.operands[1]) << ");\n";
      } else if (n == "math.sqrt" || n == "math.absf" || n == "math.floor" || n == "math.ceil" || n == "math.exp" || n == "math.log" || n == "math.sin" || n == "math.cos" ||
                 n == "math.tanh") {
        if (n != "math.sqrt" && n != "math.absf" && n != "math.floor" && n != "math.ceil") saw_elementary = true;
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = neptune_hip::ops::" << n.substr(5) << "("
          << val(op.operands[0]) << ");\n";
      } else if (n == "arith.cmpf") {
        const std::string a = val(op.operands[0]), b = val(op.operands[1]), &p = op.predicate;
        std::string e;
        if (p == "oeq") e = a + " == " + b; else if (p == "ogt") e = a + " > " + b; else if (p == "oge") e = a + " >= " + b;
        else if (p == "olt") e = a + " < " + b; else if (p == "ole") e = a + " <= " + b;
        else if (p == "one") e = "(" + a + " < " + b + " || " + a + " > " + b + ")";
        else if (p == "ord") e = "(" + a + " == " + a + " && " + b + " == " + b + ")";
        else if (p == "ueq") e = "!(" + a + " < " + b + " || " + a + " > " + b + ")";
        else if (p == "ugt") e = "!(" + a + " <= " + b + ")"; else if (p == "uge") e = "!(" + a + " < " + b + ")";
        else if (p == "ult") e = "!(" + a + " >= " + b + ")"; else if (p == "ule") e = "!(" + a + " > " + b + ")";
        else if (p == "une") e = a + " != " + b; else e = "(" + a + " != " + a + " || " + b + " != " + b + ")";
        o << ind << "const bool " << res() << " = " << e << ";\n";
      } else if (n == "arith.cmpi") {
        // unsigned predicates compare the operands' bits (of their own width), signed ones their two's complement
        // values (i1 true = -1)
        const std::string &p = op.predicate, &e = op.types[0].elem;
        const bool uns = p[0] == 'u', sgn = p[0] == 's';
        std::string sym = (p == "eq") ? "==" : (p == "ne") ? "!=" : (p.substr(1) == "lt") ? "<" : (p.substr(1) == "le") ? "<="
                          : (p.substr(1) == "gt") ? ">" : ">=";
        auto operand = [&](const std::string& v) {
          return uns ? "(" + utype(e) + ")" + v : (sgn && e == "i1") ? sext(v, e) : v;
        };
        o << ind << "const bool " << res() << " = " << operand(val(op.operands[0])) << " " << sym << " "
          << operand(val(op.operands[1])) << ";\n";
      } else if (n == "arith.select") {
        o << ind << "const " << ctype(op.types[0].elem) << " " << res() << " = " << val(op.operands[0]) << " ? "
          << val(op.operands[1]) << " : " << val(op.operands[2]) << ";\n";
      } else if (n == "arith.index_cast" || n == "arith.sitofp" || n == "arith.fptosi" || n == "arith.extf" ||
                 n == "arith.truncf" || n == "arith.extsi" || n == "arith.trunci") {
        // integer sources are read sign-extended (i1 true = -1); an i1 destination keeps the low bit
        const std::string &from = op.types[0].elem, &to = op.types[1].elem;
        const bool int_from = from != "f64" && from != "f32";
        std::string x = val(op.operands[0]);
        if (int_from && from == "i1") x = sext(x, from);
        if (to == "i1")
          x = "((" + (int_from ? "(uint64_t)" + x : "(int64_t)" + x) + ") & 1u) != 0";
        else
          x = "(" + ctype(to) + ")" + x;
        o << ind << "const " << ctype(to) << " " << res() << " = " << x << ";\n";
      } else if (n == "arith.uitofp") {
        // the source's bits read as an unsigned integer of the source's width
        const std::string& from = op.types[0].elem;
        o << ind << "const " << ctype(op.types[1].elem) << " " << res() << " = (" << ctype(op.types[1].elem) << ")("
          << (from == "i1" ? std::string("bool") : utype(from)) << ")" << val(op.operands[0]) << ";\n";
      } else if (n == "scf.if") {
        for (size_t r = 0; r < op.results.size(); ++r) o << ind << ctype(op.types[r].elem) << " " << cname(op.results[r]) << ";\n";
        o << ind << "if (" << val(op.operands[0]) << ") {\n";
        if (!emit_region_ops(*op.regions[0], o, ind + "  ", temp_index, index_arg, &op.results)) return false;
        o << ind << "}";
        if (op.regions.size() > 1) {
          o << " else {\n";
          if (!emit_region_ops(*op.regions[1], o, ind + "  ", temp_index, index_arg, &op.results)) return false;
          o << ind << "}";
        }
        o << "\n";
      } else if (n == "scf.yield") {
        for (size_t r = 0; r < op.operands.size() && if_results; ++r)
          o << ind << cname((*if_results)[r]) << " = " << val(op.operands[r]) << ";\n";
      } else if (n == "neptune_ir.yield") {
        o << ind << "return " << val(op.operands[0]) << ";\n";
      } else {
        diag.fail(op.line, "cannot emit '" + n + "'");
        return false;
      }
    }
    return true;
  }

  // checks + footprint of one apply (no emission): which inputs need a ring, the shared radii on the
  // kernel's axes, whether the march kernel can take it
  bool analyze_apply(const Op& apply, Footprint& fp, std::map<std::string, int>& temp_index,
                     std::map<std::string, int>& index_arg) {
    const Block& blk = *apply.regions[0];
    const Bounds& b = apply.attrs.at("bounds").bounds;
    const int rank = b.rank();
    const int nin = (int)apply.operands.size();
    const Type& res = apply.types[nin];
    if (rank > 6) { diag.fail(apply.line, "apply of rank " + std::to_string(rank) + " (the HIP backend supports rank 1..6)"); return false; }
    if (nin > 4) { diag.fail(apply.line, "apply with more than 4 inputs"); return false; }
    if (res.elem != "f64" && res.elem != "f32") { diag.fail(apply.line, "apply element type " + res.elem + " (f64 and f32 are supported)"); return false; }
    for (int k = 0; k < nin; ++k)
      if (apply.types[k].elem != res.elem) { diag.fail(apply.line, "apply inputs of mixed element types"); return false; }
    fp = Footprint();
    fp.nin = nin;
    // rank 4..6: the leading rank-3 dimensions are batch / component dimensions -- no access may have an offset along them
    // (the kernels are rank 1..3); the host launches one rank-3 apply per leading index (run_apply_batched) and the body
    // sees the leading indices as members.  Index argument d maps to -(d+1) for a leading dimension.
    const int lead = rank > 3 ? rank - 3 : 0;
    fp.lead = lead;
    fp.rank = rank - lead;
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) { fp.radius[k][d] = 0; fp.top_radius[k][d] = -1; fp.top_lo[k][d] = 1; fp.top_hi[k][d] = -1; }
    for (int d = 0; d < rank; ++d) index_arg[blk.args[d].name] = d < lead ? -(d + 1) : d - lead;
    for (int k = 0; k < nin; ++k) temp_index[blk.args[rank + k].name] = k;
    if (lead > 0) {
      // an offset along a leading dimension makes it a stencil in more than three dimensions: the rank-generic kernel
      for (int k = 0; k < 4; ++k)
        for (int d = 0; d < 6; ++d) { fp.nd_lo[k][d] = 1; fp.nd_hi[k][d] = -1; }
      std::function<void(const Block&, bool)> scan_nd = [&](const Block& b, bool top) {
        for (auto& op : b.ops) {
          if (op->name == "neptune_ir.access") {
            const int k = temp_index.at(op->operands[0]);
            for (int d = 0; d < rank; ++d) {
              const int off = (int)op->offsets[d];
              if (d < lead && off != 0) fp.nd = true;
              if (d == 0) fp.nd_halo0 = std::max(fp.nd_halo0, std::abs(off));
              if (top) {
                if (fp.nd_hi[k][d] < fp.nd_lo[k][d]) fp.nd_lo[k][d] = fp.nd_hi[k][d] = off;
                else { fp.nd_lo[k][d] = std::min(fp.nd_lo[k][d], off); fp.nd_hi[k][d] = std::max(fp.nd_hi[k][d], off); }
              }
            }
          }
          for (auto& r : op->regions) scan_nd(*r, false);
        }
      };
      scan_nd(blk, true);
      if (fp.nd)
        for (int d = 0; d < rank; ++d) index_arg[blk.args[d].name] = d;   // every index argument through the accessor
    }
    // inputs never read unconditionally keep top_radius -1 ("not accessed": nothing to check)
    scan_accesses(blk, temp_index, fp, true);
    finish_footprint(fp, res.elem);
    return true;
  }

  // from the per-input radii (fp.radius, fp.box, fp.nin, fp.rank) to what the kernels are told: which inputs get a ring,
  // the shared radii, whether a march-class kernel holds it.  Also run on the union footprint of a group of applies.
  static void finish_footprint(Footprint& fp, const std::string& elem) {
    const int nin = fp.nin;
    // rank mapping onto the kernel's (I,J,K) axes, see apply_common.hpp AxisMap.
    // every input read at a non-zero offset gets a register ring in the march kernel; the rings share
    // the largest radii
    const int krank = fp.rank;   // the kernel's rank (the last three dimensions of a wider apply)
    int* R = fp.R;
    for (int k = 0; k < nin; ++k) {
      bool any = false;
      for (int d = 0; d < krank; ++d) any = any || fp.radius[k][d] > 0;
      if (!any) continue;
      ++fp.halo_inputs;
      fp.halo_mask |= 1u << k;
      if (fp.halo_input < 0) fp.halo_input = k;
      const int* r = fp.radius[k];
      int m[3] = {0, 0, 0};
      if (fp.rank == 3) { m[0] = r[0]; m[1] = r[1]; m[2] = r[2]; }
      else if (fp.rank == 2) { m[0] = r[0]; m[2] = r[1]; }
      else { m[2] = r[0]; }
      for (int a = 0; a < 3; ++a) R[a] = std::max(R[a], m[a]);
    }
    const int vk = 16 / esize(elem);
    // the march kernel keeps 2*R0+1 planes of RJ+2*R1 rows per halo input in registers.  3-D: radius 1 for box
    // stencils, up to 4 for stars (4th/6th/8th-order 13-, 19- and 25-point operators; the 2-row late-J-halo tile
    // holds a radius-3 ring in 209 VGPRs without scratch, a radius-4 ring in 229 with one plane in flight), at most
    // two halo inputs (one beyond radius 1).
    // 1-D / 2-D, where a plane is one row: stars up to radius 4 (8th-order operators; K neighbours beyond one lane
    // vector come through a second wave shift, so the K radius may reach two vectors), up to four halo inputs
    // (one beyond radius 2: the register rings of two wide inputs leave one wave per SIMD), boxes up to radius 2
    // (5x5 windows, one halo input).  Wider footprints use the direct kernel.
    const int rmax = fp.box ? (krank == 3 ? 1 : 2) : 4;
    const int rbig = std::max(R[0], std::max(R[1], R[2]));
    const int hmax = krank == 3 ? (rbig > 1 ? 1 : 2) : ((rbig > 2 || (fp.box && rbig > 1)) ? 1 : 4);
    fp.march_ok = fp.halo_inputs <= hmax && R[0] <= rmax && R[1] <= rmax && R[2] <= (krank == 3 ? rmax : 2 * vk) && R[2] <= 2 * vk;
    // 3-D stars of one halo input beyond that, up to radius 8 (10th- to 16th-order operators): the plane-in-LDS kernel
    // (apply_plane.hpp) keeps only the ring of own cells in registers and reads J / K neighbours from the centre plane in LDS
    if (!fp.march_ok && krank == 3 && !fp.box && fp.halo_inputs == 1 && rbig <= 8) fp.march_ok = true;
    // ... and several inputs read at offsets, a ring and an LDS window each, while two rows per lane of all rings fit the
    // registers: inputs * (2*max(R0,1)+2) <= 21 (apply_plane.hpp plane_capable)
    if (!fp.march_ok && krank == 3 && !fp.box && fp.halo_inputs >= 2 && rbig <= 8 && (R[1] > 0 || R[2] > 0) &&
        fp.halo_inputs * (2 * std::max(R[0], 1) + 2) <= 21)
      fp.march_ok = true;
    // 2-D footprints beyond that, up to radius 8 (stars and boxes, up to four inputs read at offsets): the window of a tile in
    // LDS (neptune_apply_tile2)
    if (!fp.march_ok && krank == 2 && fp.halo_inputs >= 1 && fp.halo_inputs <= 4 && rbig <= 8) fp.march_ok = true;
    // 3-D boxes of one halo input up to radius 2 (125 points): every live plane in LDS (neptune_apply_planes)
    if (!fp.march_ok && krank == 3 && fp.box && fp.halo_inputs == 1 && rbig <= 2 && R[0] >= 1) fp.march_ok = true;
    if (!fp.march_ok) { fp.halo_input = -1; fp.halo_mask = 0; R[0] = R[1] = R[2] = 0; }
  }

  // a reach table: {{most negative offset per input and dimension}, {most positive}} (hi < lo: not accessed)
  template <int D>
  static std::string reach_table(const int (&lo)[4][D], const int (&hi)[4][D]) {
    std::ostringstream o;
    o << "{";
    for (int side = 0; side < 2; ++side) {
      o << (side ? ", {" : "{");
      for (int k = 0; k < 4; ++k) {
        o << (k ? ", {" : "{");
        for (int d = 0; d < D; ++d) o << (d ? ", " : "") << (side ? hi[k][d] : lo[k][d]);
        o << "}";
      }
      o << "}";
    }
    o << "}";
    return o.str();
  }

  // reach of a fused explicit time step: the rhs body's unconditional accesses of the state, and the axpy's read of the centre
  static std::string fused_reach(const Footprint& cfp, int rank) {
    int lo[4][3], hi[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) {
        const bool state = k == 0 && d < rank;
        lo[k][d] = state ? std::min(cfp.top_lo[0][d], 0) : 1;   // an unread dimension (1, -1) widens to (0, 0)
        hi[k][d] = state ? std::max(cfp.top_hi[0][d], 0) : -1;
      }
    return reach_table(lo, hi);
  }

  // reach of an apply along dim 0 (the slab axis), over all of its accesses
  static int halo0_of(const Footprint& fp) {
    int h = 0;
    for (int k = 0; k < fp.nin; ++k) h = std::max(h, fp.radius[k][0]);
    return h;
  }

  static std::string footprint_type(const Footprint& fp) {
    std::ostringstream o;
    o << "neptune_hip::Footprint<" << fp.halo_input << ", " << fp.R[0] << ", " << fp.R[1] << ", " << fp.R[2] << ", "
      << ((fp.box && fp.march_ok) ? "true" : "false") << ", " << (fp.march_ok ? "true" : "false");
    if (fp.halo_inputs > 1 && fp.march_ok) o << ", 0x" << std::hex << fp.halo_mask << std::dec << "u";
    o << ">";
    return o.str();
  }

  bool emit_body(const Op& apply, const std::string& tag, Footprint& fp) {
    const Block& blk = *apply.regions[0];
    const int nin = (int)apply.operands.size();
    const int rank = apply.attrs.at("bounds").bounds.rank();
    const Type& res = apply.types[nin];
    std::map<std::string, int> temp_index, index_arg;
    if (!analyze_apply(apply, fp, temp_index, index_arg)) return false;
    std::ostringstream& o = bodies;
    o << "// " << tag << ": region of the neptune_ir.apply at line " << apply.line << "\n";
    o << "struct Body_" << tag << " {\n";
    if (rank > 3 && !fp.nd) o << "  int64_t lead[3] = {0, 0, 0};   // indices along the leading (batch) dimensions, set per launch\n";
    o << "  template <class A>\n  __device__ __forceinline__ " << ctype(res.elem) << " operator()(const A& a) const {\n";
    saw_elementary = false;
    nd_body = fp.nd;
    const bool body_ok = emit_region_ops(blk, o, "    ", temp_index, index_arg, nullptr);
    nd_body = false;
    if (!body_ok) return false;
    fp.exact = !saw_elementary;
    o << "  }\n};\n";
    o << "using FP_" << tag << " = " << footprint_type(fp) << ";\n";
    // what the unconditional accesses reach, per input and dimension (analyze_apply leaves hi < lo where nothing is read)
    o << "static const neptune_hip::Reach kTopRadius_" << tag << " = " << reach_table(fp.top_lo, fp.top_hi) << ";\n";
    if (fp.nd) o << "static const neptune_hip::ReachN kNdReach_" << tag << " = " << reach_table(fp.nd_lo, fp.nd_hi) << ";\n";
    o << "\n";
    return true;
  }

  // ---- functions -----------------------------------------------------------------------
  struct ValueInfo {
    int root_arg = -1;  // >= 0: aliases function argument #root_arg
    int uses = 0;
  };

  bool lowerable(const Function& f, std::string& why, int depth = 0) {
    if (depth > 32) { why = "recursive opdef calls"; return false; }
    for (auto& op : f.body.ops)
      if (op->opaque) { why = "contains '" + op->name + "' (solver / time-stepping op: stays on the host path)"; return false; }
    if (f.result_types.size() > 1) { why = "more than one result"; return false; }
    for (auto& t : f.arg_types)
      if (!(t.kind == TypeKind::MemRef || t.is_tempish())) { why = "argument of type " + t.str() + " (only memref / temp / field arguments are lowered)"; return false; }
    for (auto& t : f.result_types)
      if (!(t.kind == TypeKind::MemRef || t.is_tempish() || (t.is_scalar() && (t.elem == "f64" || t.elem == "f32")))) {
        why = "result of type " + t.str();
        return false;
      }
    for (auto& t : f.arg_types) {
      if (t.rank() < 1 || t.rank() > 6) { why = "rank " + std::to_string(t.rank()) + " argument"; return false; }
      if (t.elem != "f64" && t.elem != "f32") { why = "element type " + t.elem; return false; }
    }
    // every callee must be lowerable too
    for (auto& op : f.body.ops)
      if (!op->callee.empty()) {
        const Function* c = m.find(op->callee);
        std::string w2;
        if (!c || !lowerable(*c, w2, depth + 1)) { why = "calls @" + op->callee + " which is not lowered"; return false; }
      }
    return true;
  }

  struct FusedReduce {
    std::string tag, elem, result_box, bounds_box;
    int rank = 0, nin = 0, halo0 = 0;
  };

  // what the emitters of one function's ops share
  struct FnState {
    const Function& f;
    std::ostringstream o;
    std::map<std::string, ValueInfo> vals;
    std::map<std::string, FusedReduce> fused_reduce;  // apply result -> how the consuming reduce evaluates it
    std::map<std::string, int> scalar_kind;           // function-level scalars: 0 uniform, 1 bare reduce result, 2 derived from one
    int returned_scalar_kind = -1;
    std::map<int, std::string> dest_of;  // producer op index -> C expression of the destination Val*
    int returned_producer = -1;
    std::map<std::string, int> def_at;
    int apply_counter = 0;
    explicit FnState(const Function& fn) : f(fn) {}
    std::string dest_for(int oi) const {
      auto it = dest_of.find(oi);
      if (it != dest_of.end()) return it->second;
      return oi == returned_producer ? "dest" : "nullptr";
    }
  };

  // only aliases and constants lie between producer p and op oi: nothing there can observe the field p would write
  static bool nothing_observes_between(const Function& f, int p, int oi) {
    for (int j = p + 1; j < oi; ++j) {
      const std::string& nm = f.body.ops[j]->name;
      if (!is_alias_op(nm) && nm != "arith.constant") return false;
    }
    return true;
  }

  bool emit_function(const Function& f) {
    FnState s(f);
    const auto& ops = f.body.ops;
    const int nargs = (int)f.arg_types.size();
    for (int i = 0; i < nargs; ++i) s.vals[f.body.args[i].name].root_arg = i;
    for (size_t oi = 0; oi < ops.size(); ++oi) {
      for (auto& v : ops[oi]->operands) s.vals[v].uses++;
      for (auto& r : ops[oi]->results) s.def_at[r] = (int)oi;
    }
    // which producer may write straight into which destination
    auto producer_of = [&](const std::string& v) -> int {
      auto it = s.def_at.find(v);
      if (it == s.def_at.end()) return -1;
      const Op& p = *ops[it->second];
      return (p.name == "neptune_ir.apply" || !p.callee.empty()) ? it->second : -1;
    };
    for (size_t oi = 0; oi < ops.size(); ++oi) {
      const Op& op = *ops[oi];
      if (op.name == "neptune_ir.store" && !op.attrs.count("bounds")) {
        const int p = producer_of(op.operands[0]);
        const std::string& field = op.operands[1];
        const bool field_before = !s.def_at.count(field) || s.def_at[field] < p;  // function args precede everything
        if (p >= 0 && s.vals[op.operands[0]].uses == 1 && field_before && nothing_observes_between(f, p, (int)oi))
          s.dest_of[p] = "&" + cname(field);
      }
      // the caller's destination may only be handed down to a producer that is the LAST thing the function
      // computes: an op between it and the return could still read an argument that aliases that destination
      // (the reference gives every apply a private result, DataflowLowering.cpp:281)
      if (is_return_op(op.name) && op.operands.size() == 1) {
        const int p = producer_of(op.operands[0]);
        if (p >= 0 && s.vals[op.operands[0]].uses == 1 && nothing_observes_between(f, p, (int)oi)) s.returned_producer = p;
      }
    }

    std::ostringstream& o = s.o;
    o << "// ---- @" << f.name << " (line " << f.line << ") ----\n";
    o << "static nl::Val " << f.name << "__impl(nl::Scope& sc";
    for (int i = 0; i < nargs; ++i) o << ", const nl::Val& " << cname(f.body.args[i].name);
    o << ", const nl::Val* dest, int* ret_arg, double* sret) {\n";
    o << "  (void)dest; (void)sret; if (ret_arg) *ret_arg = -1;\n";
    if (s.returned_producer >= 0 && nargs > 0) {
      // ... and never when it overlaps one of this function's own arguments (checked on the actual pointers): the
      // producer would overwrite data the function was given to read
      o << "  if (dest && (";
      for (int i = 0; i < nargs; ++i) o << (i ? " || " : "") << "nl::overlaps(*dest, " << cname(f.body.args[i].name) << ")";
      o << ")) dest = nullptr;\n";
    }
    for (size_t oi = 0; oi < ops.size(); ++oi) {
      const Op& op = *ops[oi];
      const std::string& n = op.name;
      bool ok = true;
      if (is_alias_op(n)) emit_alias(s, op);
      else if (n == "neptune_ir.apply") {
        Group grp;
        if (find_group(s, (int)oi, grp)) {
          ok = emit_group(s, grp);
          oi = (size_t)grp.members.back();   // the aliases and constants between the members were emitted with the group
        } else {
          ok = emit_apply(s, op, (int)oi);
        }
      }
      else if (n == "neptune_ir.time_advance") ok = emit_time_advance(s, op, (int)oi);
      else if (!op.callee.empty()) emit_call(s, op, (int)oi);
      else if (n == "neptune_ir.store") emit_store(s, op);
      else if (n == "neptune_ir.reduce") emit_reduce(s, op);
      else if (is_scalar_op(op)) ok = emit_scalar(s, op);
      else if (is_return_op(n)) emit_return(s, op);
      if (!ok) return false;
    }
    o << "}\n";
    emit_abi(s);
    return true;
  }

  // the report entry of an apply; halo_input is star / box also when the direct kernel runs it
  ApplyInfo apply_info(const FnState& s, const std::string& tag, const Footprint& fp, int rank, const std::string& elem, int halo0) {
    ApplyInfo ai;
    ai.function = s.f.name;
    ai.tag = tag;
    ai.rank = rank;
    ai.num_inputs = fp.nin;
    ai.march = fp.march_ok;
    ai.box = fp.box;
    ai.halo_input = fp.halo_inputs > 0 ? std::max(fp.halo_input, 0) : -1;
    ai.elem = elem;
    ai.halo0 = halo0;
    ai.exact = fp.exact;
    return ai;
  }

  // const nl::Val* in_<tag>[] = {...}: the inputs of one run_apply*, as C expressions of nl::Val
  static void emit_inputs(std::ostream& o, const std::string& tag, const std::vector<std::string>& ins) {
    o << "  const nl::Val* in_" << tag << "[] = {";
    for (size_t k = 0; k < ins.size(); ++k) o << (k ? ", " : "") << "&" << ins[k];
    o << "};\n";
  }

  // Geometry-level entries of an apply body: what neptune_hip_apply_builtin is for the library's own bodies
  // (caller-supplied boxes, bounds, region, stream and launch configuration; no allocation, no synchronisation).
  // The slab decomposition drives user stencils through them.
  void emit_geom_entries(const std::string& sym, const std::string& reach, const std::string& body, const std::string& init,
                         const std::string& T, int rank, int nin, const std::string& fp, bool norm = false, bool dot = false) {
    static const char* const suffix[3] = {"", "2", "3"};
    static const char* const launch[3] = {"launch_apply", "launch_apply_twice", "launch_apply_thrice"};
    for (int v = 0; v < 3; ++v) {
      if (v == 1)
        geom_entries << "// two chained applies of this body in one pass over HBM (csrc/kernels/apply_march2.hpp): out = A(A(in)), or\n"
                     << "// NEPTUNE_HIP_EUNSUPPORTED when the footprint / geometry does not qualify (neptune_hip_step_loop_pairs)\n";
      geom_entries << "extern \"C\" int " << sym << suffix[v]
                   << "(const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* stream,\n"
                   << "    const neptune_hip_launch_cfg_t* cfg) {\n"
                   << "  if (!g || !in || !out) return NEPTUNE_HIP_EINVAL;\n"
                   << "  const int rc = neptune_hip::geom_check_radius(g, " << reach << ");\n"
                   << "  if (rc != NEPTUNE_HIP_OK) return rc;\n"
                   << "  // an output that overlaps an input is refused, as neptune_hip_apply_builtin does\n"
                   << "  if (neptune_hip::check_no_alias(g, in, out, sizeof(" << T << ")) != NEPTUNE_HIP_OK) return NEPTUNE_HIP_EINVAL;\n"
                   << "  return neptune_hip::" << launch[v] << "<" << body << ", " << T << ", " << rank << ", " << nin << ", " << fp
                   << ">(" << body << "{" << init << "}, g, in, out, (hipStream_t)stream, cfg);\n}\n";
    }
    if (norm)
      geom_entries << "// the monitored launch (lowering option norm-entries; neptune_hip_apply_norm_fn, include/neptune_hip.h): the apply and\n"
                   << "// S = sum (new - old)^2 over apply.bounds x launch region into *sum_out, or NEPTUNE_HIP_EUNSUPPORTED, nothing launched\n"
                   << "extern \"C\" int " << sym << "N(const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* sum_out,\n"
                   << "    void* stream, const neptune_hip_launch_cfg_t* cfg) {\n"
                   << "  if (!g || !in || !out || !sum_out) return NEPTUNE_HIP_EINVAL;\n"
                   << "  const int rc = neptune_hip::geom_check_radius(g, " << reach << ");\n"
                   << "  if (rc != NEPTUNE_HIP_OK) return rc;\n"
                   << "  if (neptune_hip::check_no_alias(g, in, out, sizeof(" << T << ")) != NEPTUNE_HIP_OK) return NEPTUNE_HIP_EINVAL;\n"
                   << "  return neptune_hip::launch_apply_norm<" << body << ", " << T << ", " << rank << ", " << nin << ", " << fp
                   << ">(" << body << "{" << init << "}, g, in, out, sum_out, (hipStream_t)stream, cfg);\n}\n";
    if (dot)
      geom_entries << "// the dot-monitored launch (lowering option dot-entries; neptune_hip_apply_dot_fn, include/neptune_hip.h): the apply and\n"
                   << "// D = sum new * in[0] over apply.bounds x launch region into *dot_out, or NEPTUNE_HIP_EUNSUPPORTED, nothing launched\n"
                   << "extern \"C\" int " << sym << "D(const neptune_hip_apply_geom_t* g, const void* const* in, void* out, void* dot_out,\n"
                   << "    void* stream, const neptune_hip_launch_cfg_t* cfg) {\n"
                   << "  if (!g || !in || !out || !dot_out) return NEPTUNE_HIP_EINVAL;\n"
                   << "  const int rc = neptune_hip::geom_check_radius(g, " << reach << ");\n"
                   << "  if (rc != NEPTUNE_HIP_OK) return rc;\n"
                   << "  if (neptune_hip::check_no_alias(g, in, out, sizeof(" << T << ")) != NEPTUNE_HIP_OK) return NEPTUNE_HIP_EINVAL;\n"
                   << "  return neptune_hip::launch_apply_dot<" << body << ", " << T << ", " << rank << ", " << nin << ", " << fp
                   << ">(" << body << "{" << init << "}, g, in, out, dot_out, (hipStream_t)stream, cfg);\n}\n";
    geom_entries << "// march tiles this module holds for that entry (plan-time tuning: neptune_hip_autotune_fn)\n"
                 << "extern \"C\" int " << sym << "_variants(int rank) { return neptune_hip::march_variant_count(rank); }\n\n";
  }

  // Lowering option norm-entries: an apply whose input 0 has the result's element type and a box equal to the result's --
  // the old state of an iteration u <- A(u) -- also exports its monitored launch <geom_symbol>N
  bool norm_entries = false;
  bool dot_entries = false;    // lowering option dot-entries: the same eligibility, <geom_symbol>D
  bool reduce_kinds = false;   // lowering option reduce-kinds: reduces go through the kind-taking runtime forms
  static bool monitor_eligible(const Op& op) {
    const int nin = (int)op.operands.size();
    const Type& res = op.types[nin];
    return op.types[0].elem == res.elem && op.types[0].bounds == res.bounds;
  }
  bool wants_norm_entry(const Op& op) const { return norm_entries && monitor_eligible(op); }
  bool wants_dot_entry(const Op& op) const { return dot_entries && monitor_eligible(op); }

  // A two-level scheme u(n+1) = B(u(n), u(n-1), c...) the chain kernel can step twice per pass: input 0 a star of radius
  // 1..2 per axis (what march2_footprint / march2_rank2_footprint of csrc/kernels/apply_march2.hpp take), input 1 -- the
  // previous state -- of input 0's and the result's element type, every input but input 0 read at the centre only.
  static bool leapfrog_capable(const Footprint& fp, const Op& op) {
    const int nin = (int)op.operands.size();
    if (nin < 2 || fp.lead > 0 || fp.nd || !fp.march_ok || fp.box || fp.halo_mask != 1u) return false;
    const Type& res = op.types[nin];
    if (op.types[0].elem != res.elem || op.types[1].elem != res.elem) return false;
    auto in12 = [](int r) { return r >= 1 && r <= 2; };
    // rank 3 stops where the kernel's window would need scratch memory (leapfrog2_footprint): radius 2 takes no further
    // input, radius 1 one
    if (fp.rank == 3) return in12(fp.R[0]) && in12(fp.R[1]) && in12(fp.R[2]) && nin <= (std::max(fp.R[0], std::max(fp.R[1], fp.R[2])) > 1 ? 2 : 3);
    if (fp.rank == 2) return in12(fp.R[0]) && fp.R[1] == 0 && in12(fp.R[2]);
    return false;
  }

  // <sym>L2: one leapfrog pair of that apply (neptune_hip_leapfrog2_fn, include/neptune_hip.h)
  void emit_leapfrog_entry(const std::string& sym, const std::string& reach, const std::string& body, const std::string& T, int rank,
                           int nin, const std::string& fp) {
    geom_entries << "// two steps of this two-level scheme in one pass over HBM (csrc/kernels/apply_march2.hpp, leapfrog form):\n"
                 << "// out_v = B(in[0], in[1], in[2..]), out_w = B(out_v, in[0], in[2..]); NEPTUNE_HIP_EUNSUPPORTED when the geometry or\n"
                 << "// the buffers do not qualify (neptune_hip_step_loop_leapfrog)\n"
                 << "extern \"C\" int " << sym << "L2(const neptune_hip_apply_geom_t* g, const void* const* in, void* out_v, void* out_w,\n"
                 << "    void* stream, const neptune_hip_launch_cfg_t* cfg) {\n"
                 << "  if (!g || !in || !out_v || !out_w) return NEPTUNE_HIP_EINVAL;\n"
                 << "  const int rc = neptune_hip::geom_check_radius(g, " << reach << ");\n"
                 << "  if (rc != NEPTUNE_HIP_OK) return rc;\n"
                 << "  return neptune_hip::launch_apply_leapfrog2<" << body << ", " << T << ", " << rank << ", " << nin << ", " << fp
                 << ">(" << body << "{}, g, in, out_v, out_w, (hipStream_t)stream, cfg);\n}\n\n";
  }

  void emit_alias(FnState& s, const Op& op) {
    s.vals[op.results[0]].root_arg = s.vals[op.operands[0]].root_arg;
    const bool temp = op.types[1].is_tempish();
    Bounds b = op.types[temp ? 1 : 0].bounds;
    if (!temp)  // unwrap -> memref: same buffer, zero-based box
      for (int d = 0; d < b.rank(); ++d) { b.ub[d] -= b.lb[d]; b.lb[d] = 0; }
    s.o << "  // " << op.name << " " << op.operands[0] << "\n";
    s.o << "  const nl::Val " << cname(op.results[0]) << " = sc.alias(" << cname(op.operands[0]) << ", " << new_box(b) << ", \""
        << op.name << "\");\n";
  }

  // single-use result consumed by a reduce a few scalar/alias ops later: the apply is evaluated
  // inside the reduction kernel (run_apply_reduce_sum), the temp never exists
  static const Op* fused_reduce_consumer(FnState& s, const Op& op, int oi) {
    const auto& ops = s.f.body.ops;
    if (s.vals[op.results[0]].uses != 1) return nullptr;
    for (size_t j = oi + 1; j < ops.size(); ++j) {
      const Op& c = *ops[j];
      if (c.name == "neptune_ir.reduce" && c.operands.at(0) == op.results[0]) return &c;
      const std::string& nm = c.name;
      if (!(nm == "neptune_ir.wrap" || nm == "neptune_ir.unwrap" || nm == "neptune_ir.load" || is_scalar_op(c))) break;
    }
    return nullptr;
  }
  static bool feeds_fused_reduce(FnState& s, const Op& op, int oi) { return fused_reduce_consumer(s, op, oi) != nullptr; }

  // group >= 0: the apply is a member of that group -- its body functor, geometry-level entries and report entry are
  // what they are for an apply on its own; the launch itself is emitted by emit_group
  bool emit_apply(FnState& s, const Op& op, int oi, int group = -1, std::string* tag_out = nullptr) {
    const std::string tag = s.f.name + "_" + std::to_string(s.apply_counter++);
    if (tag_out) *tag_out = tag;
    Footprint fp;
    if (!emit_body(op, tag, fp)) return false;
    const int nin = (int)op.operands.size();
    const Type& res = op.types[nin];
    ValueInfo& vi = s.vals[op.results[0]];
    vi.root_arg = -1;
    const bool fused = group < 0 && fp.lead == 0 && feeds_fused_reduce(s, op, oi);
    if (group >= 0) {
      ApplyInfo ai = apply_info(s, tag, fp, fp.rank, res.elem, halo0_of(fp));
      ai.group = group;
      ai.geom_symbol = tag + "__geom";
      if (wants_norm_entry(op)) ai.norm_symbol = ai.geom_symbol + "N";
      if (wants_dot_entry(op)) ai.dot_symbol = ai.geom_symbol + "D";
      emit_geom_entries(ai.geom_symbol, "kTopRadius_" + tag, "Body_" + tag, "", ctype(res.elem), res.bounds.rank(), nin, "FP_" + tag,
                        !ai.norm_symbol.empty(), !ai.dot_symbol.empty());
      if (leapfrog_capable(fp, op)) {
        ai.leapfrog_symbol = ai.geom_symbol + "L2";
        emit_leapfrog_entry(ai.geom_symbol, "kTopRadius_" + tag, "Body_" + tag, ctype(res.elem), res.bounds.rank(), nin, "FP_" + tag);
      }
      info.applies.push_back(ai);
      return true;
    }
    const std::string res_box = new_box(res.bounds), bounds_box = new_box(op.attrs.at("bounds").bounds);
    std::vector<std::string> ins;
    for (auto& v : op.operands) ins.push_back(cname(v));
    s.o << "  // neptune_ir.apply -> " << op.results[0]
        << (fused ? "   (evaluated inside the reduce below)\n" : "   (kernel + fused copy-through)\n");
    emit_inputs(s.o, tag, ins);
    if (fused) {
      s.fused_reduce[op.results[0]] = {tag, ctype(res.elem), res_box, bounds_box, res.bounds.rank(), nin, halo0_of(fp)};
      ApplyInfo ai = apply_info(s, tag, fp, fp.rank, "", 0);
      ai.march = false;
      ai.fused_reduce = true;
      if (reduce_kinds) ai.reduce_kind = fused_reduce_consumer(s, op, oi)->attrs.at("kind").s;
      info.applies.push_back(ai);
      return true;
    }
    // the run_apply* template arguments and call arguments the three forms share
    const std::string targs = "<Body_" + tag + ", " + ctype(res.elem) + ", " + std::to_string(res.bounds.rank()) + ", " +
                              std::to_string(nin);
    const std::string args = "(sc, Body_" + tag + "{}, " + res_box + ", " + bounds_box + ", in_" + tag + ", ";
    const std::string dest = s.dest_for(oi);
    s.o << "  const nl::Val " << cname(op.results[0]) << " = ";
    // rank 4..6: no geometry-level entry (neptune_hip_apply_geom_t is rank 1..3)
    if (fp.nd) {
      // offsets along a leading dimension: the rank-generic kernel (lowered_runtime.hpp run_apply_nd)
      s.o << "nl::run_apply_nd" << targs << ">" << args << "kNdReach_" << tag << ", " << dest << ", " << fp.nd_halo0 << ");\n";
      ApplyInfo ai = apply_info(s, tag, fp, res.bounds.rank(), res.elem, fp.nd_halo0);
      ai.march = false;
      ai.box = true;
      ai.halo_input = 0;
      info.applies.push_back(ai);
    } else if (fp.lead > 0) {
      // one rank-3 apply per index of the leading dimensions (lowered_runtime.hpp run_apply_batched)
      s.o << "nl::run_apply_batched" << targs << ", FP_" << tag << ">" << args << "kTopRadius_" << tag << ", " << dest << ");\n";
      info.applies.push_back(apply_info(s, tag, fp, res.bounds.rank(), res.elem, 0));
    } else {
      s.o << "nl::run_apply" << targs << ", FP_" << tag << ">" << args << "kTopRadius_" << tag << ", " << dest << ", "
          << halo0_of(fp) << ");\n";
      ApplyInfo ai = apply_info(s, tag, fp, fp.rank, res.elem, halo0_of(fp));
      ai.geom_symbol = tag + "__geom";
      if (wants_norm_entry(op)) ai.norm_symbol = ai.geom_symbol + "N";
      if (wants_dot_entry(op)) ai.dot_symbol = ai.geom_symbol + "D";
      emit_geom_entries(ai.geom_symbol, "kTopRadius_" + tag, "Body_" + tag, "", ctype(res.elem), res.bounds.rank(), nin, "FP_" + tag,
                        !ai.norm_symbol.empty(), !ai.dot_symbol.empty());
      if (leapfrog_capable(fp, op)) {
        ai.leapfrog_symbol = ai.geom_symbol + "L2";
        emit_leapfrog_entry(ai.geom_symbol, "kTopRadius_" + tag, "Body_" + tag, ctype(res.elem), res.bounds.rank(), nin, "FP_" + tag);
      }
      info.applies.push_back(ai);
    }
    return true;
  }

  // ---- groups: sibling applies over shared inputs -> one multi-output launch (csrc/kernels/apply_common.hpp GroupBody) ----
  struct Group {
    std::vector<int> members;            // op indices of the member applies, in order
    std::vector<std::string> inputs;     // union of their operands (SSA names), in order of first use
    Footprint fp;                        // union footprint over `inputs`
    bool no_group_form = false;          // the union is planned onto a kernel without a group form: runs member by member
  };

  // A group starting at the apply ops[first]: consecutive applies with nothing between them but aliases and scalar
  // constants (no store: a load does not snapshot, a store in between could feed a later member through memory), none
  // reading another's result, same rank (1..3) / element type / result box / apply.bounds, every member's input 0 in the
  // result's box, at most 4 distinct operands of which one at least is read by two members, 2..4 members, none feeding a
  // fused reduce, none with batch dimensions or an n-D footprint.  The longest such prefix is taken.
  bool find_group(FnState& s, int first, Group& grp) {
    const auto& ops = s.f.body.ops;
    const Op& a0 = *ops[first];
    const int nin0 = (int)a0.operands.size();
    const Type& res0 = a0.types[nin0];
    const Bounds& bnd0 = a0.attrs.at("bounds").bounds;
    std::set<std::string> tainted;                 // member results and their aliases
    std::vector<Footprint> fps;
    std::vector<std::string> inputs;
    bool shared = false;
    std::vector<int> members;
    for (int j = first; j < (int)ops.size() && members.size() < 4; ++j) {
      const Op& op = *ops[j];
      if (is_alias_op(op.name) || op.name == "arith.constant") {
        bool reads_member = false;
        for (auto& v : op.operands) reads_member = reads_member || tainted.count(v);
        if (reads_member) break;
        continue;
      }
      if (op.name != "neptune_ir.apply") break;
      const int nin = (int)op.operands.size();
      if (nin < 1 || nin > 4) break;
      const Type& res = op.types[nin];
      const Bounds& bnd = op.attrs.at("bounds").bounds;
      if (bnd.rank() < 1 || bnd.rank() > 3 || res.elem != res0.elem || !(res.bounds == res0.bounds) || !(bnd == bnd0)) break;
      if (!(op.types[0].bounds == res.bounds) || !op.types[0].is_tempish()) break;
      if (res.elem != "f64" && res.elem != "f32") break;
      bool bad = false;
      for (int k = 0; k < nin; ++k) bad = bad || tainted.count(op.operands[k]) || op.types[k].elem != res.elem;
      if (bad || feeds_fused_reduce(s, op, j)) break;
      Footprint fp;
      std::map<std::string, int> ti, ia;
      if (!analyze_apply(op, fp, ti, ia)) return false;   // the same diagnostic emit_apply would give
      if (fp.lead > 0 || fp.nd) break;
      std::vector<std::string> next = inputs;
      bool shares = false;
      for (auto& v : op.operands) {
        if (std::find(next.begin(), next.end(), v) == next.end()) next.push_back(v);
        else if (std::find(inputs.begin(), inputs.end(), v) != inputs.end()) shares = true;
      }
      if (next.size() > 4) break;
      inputs = next;
      shared = shared || shares;
      members.push_back(j);
      fps.push_back(fp);
      tainted.insert(op.results[0]);
    }
    // a member that shares nothing with the ones before it may still be followed by one that does; a group needs one
    // shared value in all
    if (members.size() < 2 || !shared) return false;
    // union footprint: per group input the largest radius any member reads it at, a box if any member's is
    Footprint u;
    u.nin = (int)inputs.size();
    u.rank = fps[0].rank;
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) { u.radius[k][d] = 0; u.top_radius[k][d] = -1; u.top_lo[k][d] = 1; u.top_hi[k][d] = -1; }
    bool any_march = false;
    for (size_t m = 0; m < members.size(); ++m) {
      const Op& op = *ops[members[m]];
      any_march = any_march || fps[m].march_ok;
      u.box = u.box || fps[m].box;
      for (size_t k = 0; k < op.operands.size(); ++k) {
        const int gi = (int)(std::find(inputs.begin(), inputs.end(), op.operands[k]) - inputs.begin());
        for (int d = 0; d < 3; ++d) u.radius[gi][d] = std::max(u.radius[gi][d], fps[m].radius[k][d]);
      }
    }
    finish_footprint(u, res0.elem);
    // a union no march-class kernel holds while a member alone runs on one: fusing would trade a fast launch for a slow one
    if (!u.march_ok && any_march) return false;
    // what the march kernel's registers do not hold runs on the LDS kernels, which have no group form
    // (apply_launch.hpp plane_only / tile2_only): the runtime then runs the members one by one
    const int rbig = std::max(u.R[0], std::max(u.R[1], u.R[2]));
    if (u.march_ok)
      grp.no_group_form = u.rank == 3 ? (rbig > 1 || u.halo_inputs > 2) : (u.rank == 2 ? (rbig > 2 || (u.box && rbig > 1)) : false);
    grp.members = members;
    grp.inputs = inputs;
    grp.fp = u;
    return true;
  }

  bool emit_group(FnState& s, const Group& grp) {
    const auto& ops = s.f.body.ops;
    const int gidx = (int)info.groups.size();
    const int first = grp.members.front(), last = grp.members.back();
    const Op& a0 = *ops[first];
    const Type& res = a0.types[a0.operands.size()];
    const std::string T = ctype(res.elem);
    const int rank = res.bounds.rank(), M = (int)grp.members.size(), NU = (int)grp.inputs.size();
    // the aliases and constants between the members first: none of them reads a member's result
    std::vector<std::string> tags(M);
    for (int j = first, m = 0; j <= last; ++j) {
      const Op& op = *ops[j];
      if (is_alias_op(op.name)) emit_alias(s, op);
      else if (op.name == "arith.constant") { if (!emit_scalar(s, op)) return false; }
      else { if (!emit_apply(s, op, j, gidx, &tags[m])) return false; ++m; }
    }
    const std::string gtag = tags[0] + "_group";
    // destinations: member m may write straight into the field its single consumer stores it to when only aliases,
    // constants and the other members' own such stores lie between the group and that store (the runtime checks the
    // actual pointers against every input and every other destination); else what the apply on its own would get
    std::vector<std::string> dest(M), dest_single(M);
    for (int m = 0; m < M; ++m) dest[m] = dest_single[m] = s.dest_for(grp.members[m]);
    for (int j = last + 1; j < (int)ops.size(); ++j) {
      const Op& op = *ops[j];
      if (is_alias_op(op.name) || op.name == "arith.constant") continue;
      if (op.name != "neptune_ir.store" || op.attrs.count("bounds")) break;
      int m = -1;
      for (int k = 0; k < M; ++k)
        if (ops[grp.members[k]]->results[0] == op.operands[0]) m = k;
      const std::string& field = op.operands[1];
      const bool field_before = !s.def_at.count(field) || s.def_at[field] < first;
      if (m < 0 || s.vals[op.operands[0]].uses != 1 || !field_before) break;
      dest[m] = "&" + cname(field);
    }
    // the group body: members with their footprints and the map from member input to group input
    std::ostringstream gb, init;
    gb << "neptune_hip::GroupBody<" << T;
    for (int m = 0; m < M; ++m) {
      const Op& op = *ops[grp.members[m]];
      gb << ", neptune_hip::GroupMember<Body_" << tags[m] << ", FP_" << tags[m] << ", " << op.operands.size();
      for (auto& v : op.operands) gb << ", " << (std::find(grp.inputs.begin(), grp.inputs.end(), v) - grp.inputs.begin());
      gb << ">";
    }
    gb << ">";
    std::ostringstream& o = s.o;
    o << "  // group of " << M << " sibling applies over " << NU << " shared inputs -> one multi-output launch (members:";
    for (int m = 0; m < M; ++m) o << " " << ops[grp.members[m]]->results[0];
    o << ")\n";
    // the group's types and its members' reach tables at file scope: the lowered function and the group's geometry-level
    // entry launch the same instantiations
    bodies << "// " << gtag << ": " << M << " sibling applies over " << NU << " shared inputs as one GroupBody\n"
           << "using Group_" << gtag << " = " << gb.str() << ";\n"
           << "using FP_" << gtag << " = " << footprint_type(grp.fp) << ";\n"
           << "static const neptune_hip::Reach* const reach_" << gtag << "[] = {";
    for (int m = 0; m < M; ++m) bodies << (m ? ", " : "") << "&kTopRadius_" << tags[m];
    bodies << "};\n\n";
    std::vector<std::string> ins;
    for (auto& v : grp.inputs) ins.push_back(cname(v));
    emit_inputs(o, gtag, ins);
    auto list = [&](const char* type, const std::string& name, const std::vector<std::string>& items) {
      o << "  " << type << " " << name << "_" << gtag << "[] = {";
      for (size_t k = 0; k < items.size(); ++k) o << (k ? ", " : "") << items[k];
      o << "};\n";
    };
    std::vector<std::string> halo0;
    for (int m = 0; m < M; ++m) {
      Footprint fp;
      std::map<std::string, int> ti, ia;
      if (!analyze_apply(*ops[grp.members[m]], fp, ti, ia)) return false;
      halo0.push_back(std::to_string(halo0_of(fp)));
    }
    list("const int", "halo0", halo0);
    list("const nl::Val* const", "dest", dest);
    list("const nl::Val* const", "dest1", dest_single);
    o << "  nl::Val out_" << gtag << "[" << M << "];\n";
    o << "  nl::run_apply_group<Group_" << gtag << ", " << T << ", " << rank << ", " << NU << ", FP_" << gtag << ">(sc, Group_" << gtag
      << "{}, " << new_box(res.bounds) << ", " << new_box(a0.attrs.at("bounds").bounds) << ", in_" << gtag << ", reach_" << gtag
      << ", halo0_" << gtag << ", dest_" << gtag << ", dest1_" << gtag << ", out_" << gtag << ");\n";
    for (int m = 0; m < M; ++m)
      o << "  const nl::Val " << cname(ops[grp.members[m]]->results[0]) << " = out_" << gtag << "[" << m << "];\n";
    GroupInfo gi;
    gi.function = s.f.name;
    gi.members = tags;
    gi.inputs = grp.inputs;
    gi.kernel = grp.no_group_form ? "members" : (grp.fp.march_ok ? "march" : "direct");
    gi.rank = rank;
    gi.elem = res.elem;
    gi.geom_symbol = gtag + "__geom";
    for (int m = 0; m < M; ++m) {
      const std::string& own = ops[grp.members[m]]->operands[0];
      gi.through.push_back((int)(std::find(grp.inputs.begin(), grp.inputs.end(), own) - grp.inputs.begin()));
    }
    info.groups.push_back(gi);
    // The group's geometry-level entry (neptune_hip_group_fn, include/neptune_hip.h): what <tag>__geom is for one apply.
    // One fused launch, or the members' own launches where the fused form does not apply (apply_launch.hpp
    // apply_group_geom); it instantiates no kernel the lowered function does not.
    geom_entries << "// group of " << M << " applies over " << NU << " inputs: g describes the union inputs, out[m] is member m's result\n"
                 << "extern \"C\" int " << gi.geom_symbol << "(const neptune_hip_apply_geom_t* g, const void* const* in, void* const* out,\n"
                 << "    void* stream, const neptune_hip_launch_cfg_t* cfg) {\n"
                 << "  return neptune_hip::apply_group_geom<Group_" << gtag << ", " << T << ", " << rank << ", " << NU << ", FP_" << gtag
                 << ">(Group_" << gtag << "{}, g, in, out, (hipStream_t)stream, cfg, reach_" << gtag << ");\n}\n\n";
    return true;
  }

  // the rhs apply of a time_advance that one kernel can fuse with the axpy: the opdef is exactly "apply(state) ; return"
  // with result box == state box (nullptr: two kernels)
  const Op* fusable_rhs(const Op& op) const {
    const Type& st = op.types[0];
    const Function* c = m.find(op.callee);
    if (!(st.rank() <= 3 && c && c->arg_types.size() == 1 && c->body.ops.size() == 2 && c->body.ops[0]->name == "neptune_ir.apply" &&
          c->body.ops[1]->name == "neptune_ir.return" && c->body.ops[1]->operands.size() == 1 &&
          c->body.ops[1]->operands[0] == c->body.ops[0]->results.at(0) && c->body.ops[0]->operands.size() == 1 &&
          c->body.ops[0]->operands[0] == c->body.args[0].name))
      return nullptr;
    const Op& a = *c->body.ops[0];
    const Type &in = a.types[0], &rt = a.types[1];
    const bool same = in.is_tempish() && in.elem == st.elem && rt.elem == st.elem && in.bounds == st.bounds && rt.bounds == st.bounds;
    return same ? &a : nullptr;
  }

  // explicit Euler step: k = rhs(state); result = state + dt * k, over the whole box.  The
  // reference's own explicit lowering (HighLevelConvertion.cpp:77-120) builds exactly this
  // apply_{linear,nonlinear} + axpy apply pair (its version is 1-D-only and ill-formed).
  // A fusable rhs runs as one kernel computing state + dt * rhs(state) (ops::EulerFused); both forms produce the same bits.
  bool emit_time_advance(FnState& s, const Op& op, int oi) {
    const Type& st = op.types[0];
    s.vals[op.results[0]].root_arg = -1;
    const std::string dest = s.dest_for(oi);
    const std::string tag = s.f.name + "_ta" + std::to_string(s.apply_counter++);
    const std::string bx = new_box(st.bounds);
    const std::string T = ctype(st.elem);
    const std::string state = cname(op.operands[0]), dt = "(" + T + ")" + cname(op.operands[1]);
    std::ostringstream& o = s.o;
    const Op* rhs_apply = fusable_rhs(op);
    if (!rhs_apply) {
      o << "  // neptune_ir.time_advance {method = 0 (explicit), rhs = @" << op.callee << "}: state + dt * rhs(state)\n";
      o << "  const nl::Val k_" << tag << " = " << op.callee << "__impl(sc, " << state << ", nullptr, nullptr, nullptr);\n";
      if (st.rank() > 3) {
        // rank 4..6: the rhs through its own lowering (leading dimensions peeled off, or the rank-generic kernel), the
        // axpy as one flat pointwise pass
        o << "  const nl::Val " << cname(op.results[0]) << " = nl::run_euler_axpy_flat<" << T << ">(sc, " << dt << ", " << state
          << ", k_" << tag << ", " << dest << ");\n";
      } else {
        emit_inputs(o, tag, {state, "k_" + tag});
        const std::string axpy = "neptune_hip::ops::EulerAxpy<" + T + ", " + std::to_string(st.rank()) + ">";
        o << "  const nl::Val " << cname(op.results[0]) << " = nl::run_apply<" << axpy << ", " << T << ", " << st.rank()
          << ", 2, nl::PointwiseFP>(sc, " << axpy << "{" << dt << "}, " << bx << ", " << bx << ", in_" << tag
          << ", nl::kPointwiseRadius2, " << dest << ");\n";
      }
      Footprint pointwise;  // the axpy reads state and k at the centre
      pointwise.nin = 2;
      info.applies.push_back(apply_info(s, tag, pointwise, st.rank(), "", 0));
      return true;
    }
    Footprint cfp;
    std::map<std::string, int> ti, ia;
    if (!analyze_apply(*rhs_apply, cfp, ti, ia)) return false;
    const std::string ctag = op.callee + "_0";  // the tag emit_apply gives the opdef's only apply
    o << "  // neptune_ir.time_advance {method = 0 (explicit), rhs = @" << op.callee
      << "}: state + dt * rhs(state), rhs apply and axpy fused into one kernel\n";
    o << "  static const neptune_hip::Reach kTopRadius_" << tag << " = " << fused_reach(cfp, st.rank()) << ";\n";
    emit_inputs(o, tag, {state});
    const std::string body = "neptune_hip::ops::EulerFused<Body_" + ctag + ", " + T + ", " + std::to_string(st.rank()) + ">";
    o << "  const nl::Val " << cname(op.results[0]) << " = nl::run_apply<" << body << ", " << T << ", " << st.rank() << ", 1, FP_"
      << ctag << ">(sc, " << body << "{" << dt << "}, " << bx << ", " << new_box(rhs_apply->attrs.at("bounds").bounds) << ", in_"
      << tag << ", kTopRadius_" << tag << ", " << dest << ", " << halo0_of(cfp) << ");\n";
    ApplyInfo ai = apply_info(s, tag, cfp, st.rank(), st.elem, halo0_of(cfp));
    // With a constant time step the fused step is a self-contained apply: give it geometry-level entries too
    // (single step, two steps per pass, tile count), so step loops and slab decompositions can drive `u + dt*rhs(u)`
    // exactly like a plain operator.
    auto dit = s.def_at.find(op.operands[1]);
    const Op* dtdef = dit == s.def_at.end() ? nullptr : s.f.body.ops[dit->second].get();
    bool lit_ok = false;
    std::string lit;
    if (dtdef && dtdef->name == "arith.constant") lit = float_literal(dtdef->literal, st.elem, lit_ok);
    if (lit_ok) {
      ai.geom_symbol = tag + "__geom";
      geom_entries << "static const neptune_hip::Reach kTopRadiusG_" << tag << " = " << fused_reach(cfp, st.rank()) << ";\n";
      if (norm_entries) ai.norm_symbol = ai.geom_symbol + "N";   // the state is input 0 and the result: always eligible
      if (dot_entries) ai.dot_symbol = ai.geom_symbol + "D";
      emit_geom_entries(ai.geom_symbol, "kTopRadiusG_" + tag, body, "(" + T + ")" + lit, T, st.rank(), 1, "FP_" + ctag, norm_entries, dot_entries);
    }
    info.applies.push_back(ai);
    return true;
  }

  // apply_linear / apply_nonlinear @A(x): a call of A__impl, which may write straight into this op's destination
  void emit_call(FnState& s, const Op& op, int oi) {
    s.vals[op.results.at(0)].root_arg = -1;   // at(): a call of an opdef without a result is refused (malformed module)
    s.o << "  // " << op.name << " @" << op.callee << "\n";
    s.o << "  const nl::Val " << cname(op.results[0]) << " = " << op.callee << "__impl(sc";
    for (auto& a : op.operands) s.o << ", " << cname(a);
    s.o << ", " << s.dest_for(oi) << ", nullptr, nullptr);\n";
  }

  void emit_store(FnState& s, const Op& op) {
    s.o << "  // neptune_ir.store " << op.operands[0] << " to " << op.operands[1] << "\n";
    const std::string bx = op.attrs.count("bounds") ? "&" + new_box(op.attrs.at("bounds").bounds) : "nullptr";
    s.o << "  nl::run_store(sc, " << cname(op.operands[0]) << ", " << cname(op.operands[1]) << ", " << bx << ", "
        << dtype_macro(op.types[0].elem) << ");\n";
  }

  void emit_reduce(FnState& s, const Op& op) {
    if (reduce_kinds) return emit_reduce_kind(s, op);
    s.scalar_kind[op.results[0]] = 1;   // under a slab view: this rank's partial sum
    const std::string bx = op.attrs.count("bounds") ? "&" + new_box(op.attrs.at("bounds").bounds) : "nullptr";
    auto fit = s.fused_reduce.find(op.operands[0]);
    if (fit != s.fused_reduce.end()) {
      const FusedReduce& fr = fit->second;
      s.o << "  // neptune_ir.reduce " << op.operands[0] << " {kind = \"sum\"}   (apply + fixed-tree device sum in one kernel, blocking)\n";
      s.o << "  const " << fr.elem << " " << cname(op.results[0]) << " = (" << fr.elem << ")nl::run_apply_reduce_sum<Body_" << fr.tag
          << ", " << fr.elem << ", " << fr.rank << ", " << fr.nin << ", FP_" << fr.tag << ">(sc, Body_" << fr.tag << "{}, "
          << fr.result_box << ", " << fr.bounds_box << ", in_" << fr.tag << ", kTopRadius_" << fr.tag << ", " << fr.halo0 << ", "
          << bx << ");\n";
      return;
    }
    const std::string& elem = op.types[0].elem;
    s.o << "  // neptune_ir.reduce " << op.operands[0] << " {kind = \"sum\"}   (fixed-tree device sum, blocking)\n";
    s.o << "  const " << ctype(elem) << " " << cname(op.results[0]) << " = (" << ctype(elem) << ")nl::run_reduce_sum(sc, "
        << cname(op.operands[0]) << ", " << bx << ", " << dtype_macro(elem) << ");\n";
  }

  // lowering option reduce-kinds: every kind, "sum" included, through the kind-taking runtime forms (lowered_runtime.hpp
  // run_reduce / run_apply_reduce)
  void emit_reduce_kind(FnState& s, const Op& op) {
    const std::string& kind = op.attrs.at("kind").s;
    static const char* const macros[] = {"NEPTUNE_HIP_REDUCE_SUM", "NEPTUNE_HIP_REDUCE_MAX", "NEPTUNE_HIP_REDUCE_MIN", "NEPTUNE_HIP_REDUCE_L1",
                                         "NEPTUNE_HIP_REDUCE_L2"};
    const std::string macro = macros[reduce_kind_id(kind)];
    // under a slab view a sum is this rank's partial sum; the ranks' values of any other kind do not add up (they refuse to run)
    s.scalar_kind[op.results[0]] = kind == "sum" ? 1 : 2;
    const std::string bx = op.attrs.count("bounds") ? "&" + new_box(op.attrs.at("bounds").bounds) : "nullptr";
    auto fit = s.fused_reduce.find(op.operands[0]);
    if (fit != s.fused_reduce.end()) {
      const FusedReduce& fr = fit->second;
      s.o << "  // neptune_ir.reduce " << op.operands[0] << " {kind = \"" << kind << "\"}   (apply + fixed-tree device reduction in one kernel, blocking)\n";
      s.o << "  const " << fr.elem << " " << cname(op.results[0]) << " = (" << fr.elem << ")nl::run_apply_reduce<" << macro << ", Body_" << fr.tag
          << ", " << fr.elem << ", " << fr.rank << ", " << fr.nin << ", FP_" << fr.tag << ">(sc, Body_" << fr.tag << "{}, "
          << fr.result_box << ", " << fr.bounds_box << ", in_" << fr.tag << ", kTopRadius_" << fr.tag << ", " << fr.halo0 << ", "
          << bx << ");\n";
      return;
    }
    const std::string& elem = op.types[0].elem;
    s.o << "  // neptune_ir.reduce " << op.operands[0] << " {kind = \"" << kind << "\"}   (fixed-tree device reduction, blocking)\n";
    s.o << "  const " << ctype(elem) << " " << cname(op.results[0]) << " = (" << ctype(elem) << ")nl::run_reduce(sc, " << macro << ", "
        << cname(op.operands[0]) << ", " << bx << ", " << dtype_macro(elem) << ");\n";
  }

  // scalar arithmetic at function level (constants, reduce results): plain host statements
  bool emit_scalar(FnState& s, const Op& op) {
    static const std::map<std::string, int> none;
    if (!emit_op(op, s.o, "  ", none, none, nullptr)) return false;
    // what a scalar means when the function runs on one slab of a decomposed field: 0 = the same on every rank
    // (constants and arithmetic on them), 1 = a bare reduce result (ranks add up), 2 = computed FROM a partial sum
    // (sqrt of it, a product of two, ...): not recoverable from the per-rank values
    int kind = 0;
    for (auto& a : op.operands) {
      auto it = s.scalar_kind.find(a);
      if (it != s.scalar_kind.end() && it->second != 0) kind = 2;
    }
    for (auto& r : op.results) s.scalar_kind[r] = kind;
    return true;
  }

  void emit_return(FnState& s, const Op& op) {
    if (op.operands.empty()) {
      s.o << "  return nl::Val{};\n";
    } else if (s.f.result_types[0].is_scalar()) {
      auto it = s.scalar_kind.find(op.operands[0]);
      const int kind = it == s.scalar_kind.end() ? 0 : it->second;
      s.returned_scalar_kind = (s.returned_scalar_kind < 0 || s.returned_scalar_kind == kind) ? kind : 2;
      if (kind == 2)
        s.o << "  if (sc.has_ghosts()) nl::die(\"" << s.f.name << "\", \"slab mode: the returned scalar is computed from a reduce result, "
            << "which is only this rank's partial sum -- return the bare reduce and finish the arithmetic after the ranks' sums are added\");\n";
      s.o << "  if (sret) *sret = (double)" << cname(op.operands[0]) << ";\n  return nl::Val{};\n";
    } else {
      const int root = s.vals[op.operands[0]].root_arg;
      if (root >= 0) s.o << "  if (ret_arg) *ret_arg = " << root << ";\n";
      s.o << "  return " << cname(op.operands[0]) << ";\n";
    }
  }

  // the exported symbol with the expanded-memref ABI, and its signature in the report
  void emit_abi(FnState& s) {
    const Function& f = s.f;
    const int nargs = (int)f.arg_types.size();
    std::ostringstream& o = s.o;
    const bool has_res = !f.result_types.empty();
    const bool scalar_res = has_res && f.result_types[0].is_scalar();
    const int rrank = (has_res && !scalar_res) ? f.result_types[0].rank() : 0;
    o << "extern \"C\" "
      << (scalar_res ? ctype(f.result_types[0].elem) : has_res ? "NeptuneMemRef" + std::to_string(rrank) + "D" : std::string("void"))
      << " " << f.name << "(";
    for (int i = 0; i < nargs; ++i) {
      const int r = f.arg_types[i].rank();
      const std::string a = "a" + std::to_string(i);
      o << (i ? ", " : "") << "void* " << a << "_allocated, void* " << a << "_aligned, int64_t " << a << "_offset";
      for (int d = 0; d < r; ++d) o << ", int64_t " << a << "_size" << d;
      for (int d = 0; d < r; ++d) o << ", int64_t " << a << "_stride" << d;
    }
    o << ") {\n";
    o << "  nl::Scope sc(\"" << f.name << "\");\n";
    for (int i = 0; i < nargs; ++i) {
      const Type& t = f.arg_types[i];
      const int r = t.rank();
      const std::string a = "a" + std::to_string(i);
      o << "  const int64_t " << a << "_sizes[] = {";
      for (int d = 0; d < r; ++d) o << (d ? ", " : "") << a << "_size" << d;
      o << "}, " << a << "_strides[] = {";
      for (int d = 0; d < r; ++d) o << (d ? ", " : "") << a << "_stride" << d;
      o << "};\n";
      o << "  nl::Val m" << i << " = sc.bind_memref(" << r << ", " << esize(t.elem) << ", " << a << "_allocated, " << a
        << "_aligned, " << a << "_offset, " << a << "_sizes, " << a << "_strides);\n";
      if (t.is_tempish()) {
        // opdef arguments are temps of static shape: the descriptor must match (memref.cast ?->static)
        o << "  m" << i << " = sc.alias(m" << i << ", " << new_box(t.bounds) << ", \"argument " << i << "\");\n";
      } else {
        for (int d = 0; d < r; ++d)
          if (t.shape[d] >= 0)
            o << "  if (" << a << "_size" << d << " != " << t.shape[d] << ") nl::die(\"" << f.name << "\", \"memref argument " << i
              << " has the wrong static extent\");\n";
      }
    }
    o << "  int ret_arg = -1;\n  double sret = 0.0;\n";
    o << "  " << ((has_res && !scalar_res) ? "const nl::Val r = " : "") << f.name << "__impl(sc";
    for (int i = 0; i < nargs; ++i) o << ", m" << i;
    o << ", nullptr, &ret_arg, &sret);\n";
    o << "  sc.finish();\n";
    if (scalar_res) {
      o << "  return (" << ctype(f.result_types[0].elem) << ")sret;\n";
    } else if (has_res) {
      const std::string mr = "NeptuneMemRef" + std::to_string(rrank) + "D";
      o << "  " << mr << " out;\n";
      // result aliases an argument (e.g. @entry returns unwrap of its destination field): hand the
      // caller's own descriptor back, as the reference does (smoke_apply.mlir:23-25)
      o << "  switch (ret_arg) {\n";
      for (int i = 0; i < nargs; ++i) {
        if (f.arg_types[i].rank() != rrank) continue;
        const std::string a = "a" + std::to_string(i);
        o << "    case " << i << ": out.allocated = " << a << "_allocated; out.aligned = " << a << "_aligned; out.offset = " << a
          << "_offset;";
        for (int d = 0; d < rrank; ++d) o << " out.sizes[" << d << "] = " << a << "_size" << d << "; out.strides[" << d << "] = " << a << "_stride" << d << ";";
        o << " return out;\n";
      }
      o << "    default: break;\n  }\n";
      o << "  void* p = sc.export_result(r);\n";
      o << "  return nl::make_memref<" << rrank << ">(p, r.box);\n";
    }
    o << "}\n\n";
    funcs << o.str();
    info.lowered.push_back(f.name);
    Signature sig;
    sig.name = f.name;
    auto conv = [](const Type& t) {
      SigType st;
      st.kind = t.kind == TypeKind::MemRef ? "memref" : (t.kind == TypeKind::Temp ? "temp" : (t.is_scalar() ? "scalar" : "field"));
      st.elem = t.elem;
      st.rank = t.rank();
      if (t.kind == TypeKind::MemRef) st.shape = t.shape;
      else if (t.is_tempish()) {
        for (int d = 0; d < t.rank(); ++d) { st.shape.push_back(t.bounds.ub[d] - t.bounds.lb[d]); st.lb.push_back(t.bounds.lb[d]); }
      }
      return st;
    };
    for (auto& t : f.arg_types) sig.args.push_back(conv(t));
    sig.has_result = has_res;
    if (has_res) sig.result = conv(f.result_types[0]);
    if (scalar_res) sig.result.scalar = s.returned_scalar_kind <= 0 ? "uniform" : (s.returned_scalar_kind == 1 ? "partial_sum" : "derived");
    info.signatures.push_back(sig);
  }

  // ---- outlining: the stencil part of a function that also holds solver ops ----------------------------------
  // Every current-style input of the reference has this shape (test/smoke_tests/smoke_time_advance.mlir:53-84: @entry
  // computes %ustar with a neptune_ir.apply, then hands it to an implicit time_advance).  The solver op stays on the
  // host (RuntimeLowering, out of scope); what CAN run on the GPU is every value such an op consumes that is computed
  // by applies / operator calls from the function's own arguments.  Each becomes an exported symbol
  // <function>__stencil_<k>(<the function's memref arguments>) -> memref, with the expanded-memref ABI like any
  // lowered function, which the reference's CPU-lowered function can call in place of its scf loop nest.
  static std::unique_ptr<Op> clone_op(const Op& src) {
    auto op = std::make_unique<Op>();
    op->name = src.name; op->results = src.results; op->operands = src.operands; op->attrs = src.attrs; op->types = src.types;
    op->offsets = src.offsets; op->callee = src.callee; op->literal = src.literal; op->predicate = src.predicate;
    op->opaque = src.opaque; op->line = src.line;
    for (auto& r : src.regions) {
      auto b = std::make_unique<Block>();
      b->args = r->args;
      for (auto& o : r->ops) b->ops.push_back(clone_op(*o));
      op->regions.push_back(std::move(b));
    }
    return op;
  }
  std::vector<std::unique_ptr<Function>> outlined_funcs;   // keeps the synthetic functions alive

  void outline_stencil_parts(const Function& f, std::vector<const Function*>& todo) {
    const auto& ops = f.body.ops;
    std::map<std::string, int> def_at;
    for (size_t oi = 0; oi < ops.size(); ++oi)
      for (auto& r : ops[oi]->results) def_at[r] = (int)oi;
    // tainted: results of solver ops and everything computed from them -- and, from a store of such a value on, the
    // field it went into (and every alias of that field)
    std::map<std::string, std::string> root;   // value -> the function argument / value it aliases
    auto root_of = [&](const std::string& v) { auto it = root.find(v); return it == root.end() ? v : it->second; };
    std::map<std::string, bool> tainted;
    std::map<std::string, bool> dirty_root;
    std::vector<bool> op_tainted(ops.size(), false);
    for (size_t oi = 0; oi < ops.size(); ++oi) {
      const Op& op = *ops[oi];
      const std::string& n = op.name;
      if (is_alias_op(n))
        if (!op.results.empty() && !op.operands.empty()) root[op.results[0]] = root_of(op.operands[0]);
      bool t = op.opaque;
      for (auto& v : op.operands) t = t || tainted[v] || dirty_root[root_of(v)];
      op_tainted[oi] = t;
      for (auto& r : op.results) tainted[r] = t;
      if (t && n == "neptune_ir.store" && op.operands.size() >= 2) dirty_root[root_of(op.operands[1])] = true;
    }
    // live-outs: untainted temps produced by an apply / operator call / explicit time_advance and consumed by a tainted op
    std::vector<std::string> live;
    for (size_t oi = 0; oi < ops.size(); ++oi) {
      if (!op_tainted[oi]) continue;
      for (auto& v : ops[oi]->operands) {
        auto d = def_at.find(v);
        if (d == def_at.end() || op_tainted[d->second]) continue;
        const Op& p = *ops[d->second];
        const bool producer = p.name == "neptune_ir.apply" || !p.callee.empty();
        if (producer && std::find(live.begin(), live.end(), v) == live.end()) live.push_back(v);
      }
    }
    int k = 0;
    for (const std::string& v : live) {
      // backward slice of v over untainted ops
      std::vector<bool> need(ops.size(), false);
      std::vector<std::string> work{v};
      bool ok = true;
      while (!work.empty()) {
        const std::string x = work.back();
        work.pop_back();
        auto d = def_at.find(x);
        if (d == def_at.end()) continue;            // a function argument
        if (op_tainted[d->second]) { ok = false; break; }
        if (need[d->second]) continue;
        need[d->second] = true;
        for (auto& o : ops[d->second]->operands) work.push_back(o);
      }
      const int last = def_at[v];
      // a store before the producer could feed the slice through memory (a load of the stored field): such functions
      // are left alone rather than outlined with a side effect the caller would see twice
      for (int oi = 0; ok && oi < last; ++oi)
        if (ops[oi]->name == "neptune_ir.store") ok = false;
      if (!ok) continue;
      const Op& prod = *ops[last];
      const Type vt = prod.name == "neptune_ir.apply" ? prod.types[prod.operands.size()] : (prod.name == "neptune_ir.time_advance" ? prod.types[0] : prod.types.back());
      if (!vt.is_tempish()) continue;
      auto g = std::make_unique<Function>();
      g->name = f.name + "__stencil_" + std::to_string(k);
      g->kind = FuncKind::Func;
      g->arg_types = f.arg_types;
      g->result_types = {vt};
      g->line = prod.line;
      g->body.args = f.body.args;
      for (size_t oi = 0; oi < ops.size(); ++oi)
        if (need[oi]) g->body.ops.push_back(clone_op(*ops[oi]));
      auto ret = std::make_unique<Op>();
      ret->name = "func.return";
      ret->operands = {v};
      ret->types = {vt};
      ret->line = prod.line;
      g->body.ops.push_back(std::move(ret));
      std::string why;
      if (!lowerable(*g, why)) continue;
      info.outlined.push_back({g->name, f.name, v, prod.line});
      todo.push_back(g.get());
      outlined_funcs.push_back(std::move(g));
      ++k;
    }
  }

  // FNV-1a of the emitted constants and body functors: two modules with the same bodies share their measured launches
  static std::string module_id(const std::string& text) {
    unsigned long long h = 1469598103934665603ull;
    for (unsigned char c : text) { h ^= c; h *= 1099511628211ull; }
    char buf[32];
    snprintf(buf, sizeof buf, "%016llx", h);
    return buf;
  }

  bool run(std::string& out) {
    // callees before callers: opdefs are emitted in module order, forward declarations cover the rest
    std::ostringstream fwd;
    std::vector<const Function*> todo;
    for (auto& f : m.funcs) {
      std::string why;
      if (!lowerable(*f, why)) {
        info.skipped.push_back({f->name, why});
        outline_stencil_parts(*f, todo);    // ... but the stencil values its solver ops consume are (see above)
        continue;
      }
      todo.push_back(f.get());
    }
    for (auto* f : todo) {
      fwd << "static nl::Val " << f->name << "__impl(nl::Scope& sc";
      for (size_t i = 0; i < f->arg_types.size(); ++i) fwd << ", const nl::Val&";
      fwd << ", const nl::Val* dest, int* ret_arg, double* sret);\n";
    }
    for (auto* f : todo)
      if (!emit_function(*f)) return false;
    std::ostringstream o;
    o << "// Generated by the NeptuneIR HIP lowering (neptune-opt --neptuneir-to-hip).  Do not edit.\n"
      << "// Compile: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared <this file> \\\n"
      << "//          -I<repo> -L<repo>/neptune-pde-solver_amd/lib -lneptune_hip\n"
      << "// identifies this module's body functors in the launch-wisdom keys (include/neptune_hip.h)\n"
      << "#define NEPTUNE_HIP_MODULE_ID \"m" << module_id(consts.str() + bodies.str()) << "\"\n"
      << "#include \"neptune-pde-solver_amd/csrc/runtime/lowered_runtime.hpp\"\n"
      << "#include \"neptune-pde-solver_amd/csrc/kernels/body_ops.hpp\"\n\n"
      << "namespace nl = neptune_hip::lowered;\n\nnamespace {\n\n"
      << consts.str() << "\n"
      << bodies.str() << "}  // namespace\n\n"
      << fwd.str() << "\n"
      << funcs.str()
      << "// ---- geometry-level entries (one per apply; see include/neptune_hip.h neptune_hip_apply_builtin) ----\n"
      << geom_entries.str();
    for (auto& s : info.skipped) o << "// not lowered: @" << s.first << ": " << s.second << "\n";
    out = o.str();
    return true;
  }
};

}  // namespace

bool lower_to_hip(const Module& m, std::string& out_source, LowerInfo& info, Diag& diag, const LowerOptions& options) {
  Emitter e(m, diag, info);
  e.norm_entries = options.norm_entries;
  e.dot_entries = options.dot_entries;
  e.reduce_kinds = options.reduce_kinds;
  return e.run(out_source) && diag.ok;
}

}  // namespace neptune_lowering
