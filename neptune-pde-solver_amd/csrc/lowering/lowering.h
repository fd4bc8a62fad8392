// lowering.h -- public face of the NeptuneIR -> HIP lowering library.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "ir.h"

namespace neptune_lowering {

struct ApplyInfo {
  std::string function, tag;
  int rank = 0, num_inputs = 0, halo_input = -1;
  bool march = false, box = false;
  bool fused_reduce = false;  // evaluated inside the consuming reduce's kernel
  std::string elem;           // element type of the apply
  int halo0 = 0;              // reach along dim 0 (what a slab decomposition must hold as ghost planes)
  std::string geom_symbol;    // exported geometry-level entry (empty: none)
  std::string leapfrog_symbol;  // exported leapfrog pair entry <geom_symbol>L2 of a two-level scheme (empty: none)
  std::string norm_symbol;    // exported monitored launch <geom_symbol>N (lowering option norm-entries; empty: none)
  std::string dot_symbol;     // exported dot-monitored launch <geom_symbol>D (lowering option dot-entries; empty: none)
  std::string reduce_kind;    // fused_reduce under the lowering option reduce-kinds: the consuming reduce's kind (else empty)
  bool exact = true;          // false: the body uses elementary functions (exp, log, ...): a few ulp, not bit-exact
  int group = -1;             // index into LowerInfo::groups when this apply is a member of a group
};
// a run of sibling applies over shared inputs that one multi-output launch can compute
struct GroupInfo {
  std::string function;
  std::vector<std::string> members;   // the members' apply tags, in order
  std::vector<std::string> inputs;    // SSA names of the union of their operands, in group-input order
  std::string kernel;                 // what the union footprint is planned onto: march | direct | members (no group form)
  int rank = 0;
  std::string elem;
  std::string geom_symbol;            // exported geometry-level entry of the group, <fn>_<k0>_group__geom
  std::vector<int> through;           // per member: the group input it lists first (its unknown and copy-through source)
};
struct SigType {
  std::string kind, elem;  // kind: memref | temp | field
  int rank = 0;
  std::vector<int64_t> shape;  // -1 = dynamic
  std::vector<int64_t> lb;     // temp / field: logical origin
  // scalar results only: what the value is when the function runs on one slab of a decomposed field --
  // "uniform" (the same on every rank), "partial_sum" (a bare reduce: the ranks' values add up) or "derived"
  // (computed from a partial sum: only right on a single rank)
  std::string scalar;
};
struct Signature {
  std::string name;
  std::vector<SigType> args;
  bool has_result = false;
  SigType result;
};
struct LowerInfo {
  std::vector<Signature> signatures;                           // one per exported symbol
  std::vector<std::string> lowered;                            // exported symbols
  std::vector<std::pair<std::string, std::string>> skipped;    // (symbol, reason)
  std::vector<ApplyInfo> applies;
  std::vector<GroupInfo> groups;
  // stencil parts of functions that are not lowered as a whole (they hold solver ops): each is an exported symbol that
  // computes one value the solver op consumes, from the function's own arguments
  struct Outlined { std::string symbol, function, value; int line = 0; };
  std::vector<Outlined> outlined;
};

// What a caller may ask for beyond the default lowering.  The C ABI carries the options inside the module text, one comment
// line each -- "// neptune-hip-option: <name>" (include/neptune_lowering.h) -- so that a module's text still says everything
// about its artefact.
struct LowerOptions {
  bool norm_entries = false;   // "norm-entries": eligible applies also export their monitored launch <fn>_<k>__geomN
  bool dot_entries = false;    // "dot-entries": the same applies also export their dot-monitored launch <fn>_<k>__geomD
  bool reduce_kinds = false;   // "reduce-kinds": neptune_ir.reduce kinds max | min | l1 | l2 verify and lower
};
LowerOptions options_in_text(const char* mlir_text);   // capi.cpp

// emit_hip.cpp
bool lower_to_hip(const Module& m, std::string& out_source, LowerInfo& info, Diag& diag, const LowerOptions& options = LowerOptions());

}  // namespace neptune_lowering

// ---- C ABI (include/neptune_lowering.h documents it) ---------------------------------------
extern "C" {
int neptune_lowering_verify(const char* mlir_text, char** diag_out);
int neptune_lowering_to_hip(const char* mlir_text, char** source_out, char** report_out, char** diag_out);
int neptune_lowering_compile(const char* mlir_text, const char* so_path, const char* repo_root, const char* hipcc,
                             char** report_out, char** diag_out);
void neptune_lowering_free(char* p);
const char* neptune_lowering_version(void);
}
