// multigrid.hip -- include/neptune_hip.h: geometric multigrid over a hierarchy of applies.  Its own
// translation unit (builds in seconds, linked into libneptune_hip.so): host code plus the kernels' instantiations.
//
//   kernels alone    neptune_hip_mg_smooth, _smooth_dot, _smooth_dot_wide            the point sweep; with r . z; with the wide sum
//                    neptune_hip_mg_line_smooth, _line_first, _line_smooth_dot       one line stage: plain, apply-free, with r . z
//                    neptune_hip_mg_restrict, _restrict_linear                       a pair's restriction (Pair: which kernel)
//                    neptune_hip_mg_prolong_add, _prolong_add_linear                 a pair's prolongation
//                    neptune_hip_mg_coarsened_axes, _halved_axes                     how a pair nests
//   drivers          neptune_hip_mg_solve_transfer            V-cycles; any transfers per pair                 (Solve, run_blocks)
//                    neptune_hip_mgcg_solve_transfer          MGCG in one type; symmetric pairs only           (mgcg_drive<MgcgOneType<T>>)
//                    neptune_hip_mgcg_solve_mixed_transfer    MGCG in f64 around a cycle in f32                (mgcg_drive<MgcgMixed>)
//   forwarding       neptune_hip_mg_solve -> _solve_lines (lines = NULL) -> _solve_prolong (prolong = NULL) -> _solve_transfer
//                    (the prolong array restated as transfers with the averaging restriction);
//                    neptune_hip_mgcg_solve -> _mgcg_solve_lines (lines = NULL) -> _mgcg_solve_transfer (transfer = NULL);
//                    neptune_hip_mgcg_solve_mixed -> _mgcg_solve_mixed_transfer (transfer = NULL)
//
// Every driver runs its loop on run_blocks: blocks of check_every units (a cycle, an iteration), the first unit as plain
// launches, then ONE capture of a unit as a linear graph on the call's stream that every later unit replays; the graph is
// destroyed when the call returns.  That stream is a StreamScope's (solver_host.hpp): the one bridge stream the step loops and
// the Krylov solvers use too when the caller passes the legacy default stream.  The capture query, the read-back of device
// scalars, the outer operator of MGCG and the out-parameters' bookkeeping are that header's as well.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"   // NEPTUNE_HIP_CHECK, geom_validate, buffers_overlap (no apply kernel is instantiated here)
#include "../kernels/multigrid_kernels.hpp"
#include "../kernels/mg_line_kernels.hpp"
#include "../kernels/mgcg_kernels.hpp"
#include "../kernels/mgcg_mixed_kernels.hpp"
#include "solver_host.hpp"

using namespace neptune_hip;

namespace {

constexpr int kMaxLevels = 16;

// A level's box and Omega = apply.bounds x launch region on the kernels' three axes (the field's dimensions right-aligned);
// -> false for a malformed geometry, an input 0 in another box than the result's, or an empty Omega
bool level_box(const neptune_hip_apply_geom_t* g, MgBox& B) {
  if (!g || geom_validate(g) != NEPTUNE_HIP_OK) return false;
  for (int a = 0; a < 3; ++a) {
    B.n[a] = 1;
    B.lo[a] = 0;
    B.m[a] = 1;
  }
  for (int d = 0; d < g->rank; ++d) {
    if (g->in_lb[0][d] != g->out_lb[d] || g->in_ub[0][d] != g->out_ub[d]) return false;
    const int a = d + 3 - g->rank;
    const int64_t n = g->out_ub[d] - g->out_lb[d];
    const int64_t lo = std::max<int64_t>(std::max(g->lb[d] - g->out_lb[d], g->region_lb[d]), 0);
    const int64_t hi = std::min(std::min(g->ub[d] - g->out_lb[d], g->region_ub[d]), n);
    if (hi <= lo) return false;
    B.n[a] = n;
    B.lo[a] = lo;
    B.m[a] = hi - lo;
  }
  return true;
}
size_t box_bytes(const MgBox& B, size_t elem) { return (size_t)(B.n[0] * B.n[1] * B.n[2]) * elem; }

// How two neighbouring levels nest: per axis that carries a dimension coarsened, m_fine = 2 m_coarse + 1, halved, m_fine =
// 2 m_coarse (a cell-centred pair), or kept, m_fine = m_coarse (the three exclude each other for m >= 1).
// -> the kernels' mask (bit a: axis a is coarsened or halved), with kMgCell set when the axes are halved ones; or 0 = refuse:
// an axis in no state, none coarsened or halved, or both kinds in one pair
constexpr int kMgCell = 8;
int sizes_nest(const MgBox& F, const MgBox& Cb, int rank) {
  int coarsened = 0, halved = 0;
  for (int a = 3 - rank; a < 3; ++a) {
    if (F.m[a] == 2 * Cb.m[a] + 1) coarsened |= 1 << a;
    else if (F.m[a] == 2 * Cb.m[a]) halved |= 1 << a;
    else if (F.m[a] != Cb.m[a]) return 0;
  }
  if (coarsened && halved) return 0;
  return halved ? (halved | kMgCell) : coarsened;
}

// One pair of levels, checked: the two boxes, how they nest, and which kernel each transfer takes.  Vertex-centred or
// cell-centred by `mask`; a cell-centred pair may prolong linearly by a rule per face and restrict
// by the transpose of that prolongation, the one rule array `rim` serving both.
struct Pair {
  MgBox F, Cb;
  int rank = 0, mask = 0;                 // mask: sizes_nest's, never 0 once nest() has answered true
  bool linear = false, rlinear = false;   // the prolongation / the restriction is the linear one
  MgRim rim;                              // a linear transfer's rules on the kernels' axes (the dimensions right-aligned)

  // -> false: refuse -- the boxes do not nest.  Both transfers are the ones the pair's grid kind implies until rules() says otherwise.
  bool nest(const MgBox& fine, const MgBox& coarse, int rank_) {
    F = fine;
    Cb = coarse;
    rank = rank_;
    mask = sizes_nest(F, Cb, rank);
    linear = rlinear = false;
    for (int a = 0; a < 3; ++a) rim.lo[a] = rim.hi[a] = NEPTUNE_HIP_MG_RIM_EVEN;
    return mask != 0;
  }
  // the same from two geometries: -> false also for a malformed one and for two ranks
  bool nest(const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse) {
    MgBox fine, coarse;
    return level_box(g_fine, fine) && level_box(g_coarse, coarse) && g_fine->rank == g_coarse->rank && nest(fine, coarse, g_fine->rank);
  }
  // What the caller states about the pair's transfers, after nest(): -> false: refuse -- a prolong outside {CONSTANT, LINEAR},
  // a restrict_kind outside {AVERAGE, LINEAR}, a LINEAR transfer on a pair without a halved dimension, a rule outside {EVEN,
  // ODD} on a dimension < rank when either transfer is LINEAR.  Nothing but the two kinds is read of a CONSTANT / AVERAGE
  // entry, and no rule of a dimension >= rank.
  bool rules(const neptune_hip_mg_transfer_t& t) {
    if (t.prolong != NEPTUNE_HIP_MG_PROLONG_CONSTANT && t.prolong != NEPTUNE_HIP_MG_PROLONG_LINEAR) return false;
    if (t.restrict_kind != NEPTUNE_HIP_MG_RESTRICT_AVERAGE && t.restrict_kind != NEPTUNE_HIP_MG_RESTRICT_LINEAR) return false;
    linear = t.prolong == NEPTUNE_HIP_MG_PROLONG_LINEAR;
    rlinear = t.restrict_kind == NEPTUNE_HIP_MG_RESTRICT_LINEAR;
    if (!linear && !rlinear) return true;
    if (!(mask & kMgCell)) return false;
    for (int d = 0; d < rank; ++d) {
      for (const int32_t v : {t.rim_lo[d], t.rim_hi[d]})
        if (v != NEPTUNE_HIP_MG_RIM_EVEN && v != NEPTUNE_HIP_MG_RIM_ODD) return false;
      rim.lo[d + 3 - rank] = t.rim_lo[d];
      rim.hi[d + 3 - rank] = t.rim_hi[d];
    }
    return true;
  }
};
// a prolongation stated alone is that prolongation with the averaging restriction
neptune_hip_mg_transfer_t transfer_of(const neptune_hip_mg_prolong_t& p) {
  neptune_hip_mg_transfer_t t;
  t.prolong = p.kind;
  t.restrict_kind = NEPTUNE_HIP_MG_RESTRICT_AVERAGE;
  for (int d = 0; d < 3; ++d) {
    t.rim_lo[d] = p.rim_lo[d];
    t.rim_hi[d] = p.rim_hi[d];
  }
  return t;
}

// A field (or a scalar, or the trace) as the bytes a call touches.  align: what the address must be a multiple of;
// optional: the member may be null and is then left out of every test.
struct Span {
  const void* p;
  size_t bytes;
  size_t align = 1;
  bool optional = false;
};
// A view of some Spans, for apart()'s arguments only: it points into the braces or the array it was made from and must not
// outlive the call it is built in (a named Spans made from braces would dangle).
struct Spans {
  const Span* p;
  size_t n;
  Spans(std::initializer_list<Span> l) : p(l.begin()), n(l.size()) {}
  template <size_t N>
  Spans(const Span (&a)[N]) : p(a), n(N) {}
  Spans(const Span* p_, size_t n_) : p(p_), n(n_) {}
};
// The fields a call writes (or otherwise needs to itself) against the fields it only reads: -> false: refuse -- a member
// that is null without being optional, one that is misaligned, two of `own` that meet, one of `own` that meets one of
// `read`.  Two of `read` may meet.
bool apart(Spans own, Spans read) {
  auto sound = [](const Span& s) { return s.p ? (uintptr_t)s.p % s.align == 0 : s.optional; };
  auto meet = [](const Span& a, const Span& b) { return a.p && b.p && buffers_overlap(a.p, a.bytes, b.p, b.bytes); };
  for (size_t i = 0; i < own.n; ++i) {
    if (!sound(own.p[i])) return false;
    for (size_t o = 0; o < i; ++o)
      if (meet(own.p[i], own.p[o])) return false;
  }
  for (size_t i = 0; i < read.n; ++i) {
    if (!sound(read.p[i])) return false;
    for (size_t o = 0; o < own.n; ++o)
      if (meet(read.p[i], own.p[o])) return false;
  }
  return true;
}

// ---------------------------------------------------------------- launch geometry and dispatch
struct RowGrid {
  int64_t nchunk;
  dim3 grid;
};
// one workgroup per 256-cell chunk of a row of B's Omega
RowGrid row_grid(const MgBox& B) {
  RowGrid r;
  r.nchunk = (B.m[2] + 255) / 256;
  r.grid = grid_for_blocks(B.m[0] * B.m[1] * r.nchunk);
  return r;
}
int64_t grid_blocks(const dim3& g) { return (int64_t)g.x * g.y; }

int launched() { return hipGetLastError() == hipSuccess ? NEPTUNE_HIP_OK : NEPTUNE_HIP_EUNSUPPORTED; }

// the dispatch on element type, stated once: f(T()) with T the type
template <class Fn>
int by_type(int dtype, Fn&& f) { return dtype == NEPTUNE_HIP_F64 ? f(double()) : f(float()); }
// ... and on a pair's axes (Pair::mask & 7): launch(std::integral_constant<int, MASK>())
template <class Launch>
int by_mask(int mask, Launch&& launch) {
  switch (mask) {
    case 1: return launch(std::integral_constant<int, 1>());
    case 2: return launch(std::integral_constant<int, 2>());
    case 3: return launch(std::integral_constant<int, 3>());
    case 4: return launch(std::integral_constant<int, 4>());
    case 5: return launch(std::integral_constant<int, 5>());
    case 6: return launch(std::integral_constant<int, 6>());
    case 7: return launch(std::integral_constant<int, 7>());
    default: return NEPTUNE_HIP_EINVAL;
  }
}
template <class T>
const T* in(const void* p) { return static_cast<const T*>(p); }
template <class T>
T* io(void* p) { return static_cast<T*>(p); }

int do_smooth(int dtype, const MgBox& B, const void* q, const void* b, const void* minv, void* x, hipStream_t s) {
  const RowGrid r = row_grid(B);
  return by_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(neptune_mg_smooth<T>, r.grid, dim3(256), 0, s, B, r.nchunk, in<T>(q), in<T>(b), in<T>(minv), io<T>(x));
    return launched();
  });
}
// the sweep that also leaves one partial of b . x_new per workgroup of row_grid, in T, or -- `wide` -- on f32 fields in f64
int do_smooth_dot(int dtype, bool wide, const MgBox& B, const void* q, const void* b, const void* minv, void* x, void* partials, hipStream_t s) {
  const RowGrid r = row_grid(B);
  if (wide) {
    hipLaunchKernelGGL((neptune_mg_smooth_dot_wide<double, float>), r.grid, dim3(256), 0, s, B, r.nchunk, in<float>(q), in<float>(b),
                       in<float>(minv), io<float>(x), io<double>(partials));
    return launched();
  }
  return by_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(neptune_mg_smooth_dot<T>, r.grid, dim3(256), 0, s, B, r.nchunk, in<T>(q), in<T>(b), in<T>(minv), io<T>(x), io<T>(partials));
    return launched();
  });
}
// *out = the sum of `count` partials
int monitor_final(int dtype, const void* partials, int64_t count, void* out, hipStream_t s) {
  return by_type(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(neptune_monitor_final<T>, dim3(1), dim3(256), 0, s, in<T>(partials), count, io<T>(out));
    return launched();
  });
}

// The restriction of a pair, by the pair's choice.  The averaging ones: one workgroup per 256-cell chunk of a coarse row
// (vertex-centred with axis 2 coarsened: the fine row segments staged in LDS; kept: every lane on its own fine cells).  The
// transposed linear one: one workgroup per 256-cell chunk of a run of kMgLinearRun coarse rows of one coarse plane.
int do_restrict(int dtype, const Pair& P, const void* b_f, const void* q_f, double rscale, void* b_c, void* x_c, hipStream_t s) {
  const MgBox &F = P.F, &Cb = P.Cb;
  const RowGrid r = row_grid(Cb);
  return by_mask(P.mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    return by_type(dtype, [&](auto t) {
      using T = decltype(t);
      if (P.rlinear) {
        const int64_t nrun = (Cb.m[1] + kMgLinearRun - 1) / kMgLinearRun;
        hipLaunchKernelGGL((neptune_mg_restrict_linear<T, M>), grid_for_blocks(Cb.m[0] * nrun * r.nchunk), dim3(256), 0, s, F, Cb, r.nchunk, P.rim,
                           in<T>(b_f), in<T>(q_f), (T)rscale, io<T>(b_c), io<T>(x_c));
      } else if (P.mask & kMgCell) {
        hipLaunchKernelGGL((neptune_mg_restrict_cell<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, in<T>(b_f), in<T>(q_f), (T)rscale,
                           io<T>(b_c), io<T>(x_c));
      } else if constexpr ((M & 4) != 0) {
        hipLaunchKernelGGL((neptune_mg_restrict<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, in<T>(b_f), in<T>(q_f), (T)rscale, io<T>(b_c),
                           io<T>(x_c));
      } else {
        hipLaunchKernelGGL((neptune_mg_restrict_kept2<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, in<T>(b_f), in<T>(q_f), (T)rscale,
                           io<T>(b_c), io<T>(x_c));
      }
      return launched();
    });
  });
}
// The prolongation of a pair, by the pair's choice: one workgroup per chunk of a fine row -- 256 fine cells, but for the
// linear one 256 COARSE cells (512 fine ones) where axis 2 is halved (where it is kept, Cb.m[2] = F.m[2])
int do_prolong(int dtype, const Pair& P, const void* x_c, void* x_f, hipStream_t s) {
  const MgBox &F = P.F, &Cb = P.Cb;
  RowGrid r = row_grid(F);
  if (P.linear) {
    r.nchunk = (Cb.m[2] + 255) / 256;
    r.grid = grid_for_blocks(F.m[0] * F.m[1] * r.nchunk);
  }
  return by_mask(P.mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    return by_type(dtype, [&](auto t) {
      using T = decltype(t);
      if (P.linear)
        hipLaunchKernelGGL((neptune_mg_prolong_add_linear<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, P.rim, in<T>(x_c), io<T>(x_f));
      else if (P.mask & kMgCell)
        hipLaunchKernelGGL((neptune_mg_prolong_add_cell<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, in<T>(x_c), io<T>(x_f));
      else
        hipLaunchKernelGGL((neptune_mg_prolong_add<T, M>), r.grid, dim3(256), 0, s, F, Cb, r.nchunk, in<T>(x_c), io<T>(x_f));
      return launched();
    });
  });
}

// One stage of the line smoother along box axis `axis`.  Axis 2: a one-wave workgroup per 64 lines.  A slow axis: a workgroup
// per chunk of lanes along axis 2 and index of the other slow axis; 256 lanes wide where that still gives every CU two
// workgroups, else 64 lanes, so that a small level (a 2-D field's lines along dim 0 have m[2] / width workgroups in all)
// spreads over the CUs.  The grid is the same for the stage's three forms (kMgLinePlain, kMgLineFirst, kMgLineDot).
struct LineGrid {
  int width;        // lanes per workgroup
  int64_t nchunk;   // a slow axis: workgroups along axis 2
  dim3 grid;
};
LineGrid line_grid(const MgBox& B, int axis) {
  LineGrid L;
  if (axis == 2) {
    L.width = kMgLineGroup;
    L.nchunk = 0;
    L.grid = grid_for_blocks((B.m[0] * B.m[1] + kMgLineGroup - 1) / kMgLineGroup);
    return L;
  }
  const bool wide = B.m[1 - axis] * ((B.m[2] + 255) / 256) >= 2 * (int64_t)neptune_hip_cu_count();
  L.width = wide ? 256 : 64;
  L.nchunk = (B.m[2] + L.width - 1) / L.width;
  L.grid = grid_for_blocks(B.m[1 - axis] * L.nchunk);
  return L;
}
// the fields of one stage.  q: unused by kMgLineFirst; partials: one T per workgroup of the grid, kMgLineDot only
template <class T>
struct LineArgs {
  T* q;
  const T *b, *lo, *inv, *up;
  T *x, *partials;
};
template <class T, int MODE, int AXIS, int WIDTH>
void line_slow_launch(const MgBox& B, const LineGrid& L, const LineArgs<T>& a, hipStream_t stream) {
  if constexpr (MODE == kMgLineFirst)
    hipLaunchKernelGGL((neptune_mg_line_slow_first<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, a.b, a.lo, a.inv, a.up, a.x);
  else if constexpr (MODE == kMgLineDot)
    hipLaunchKernelGGL((neptune_mg_line_slow_dot<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, a.q, a.b, a.lo, a.inv, a.up, a.x,
                       a.partials);
  else
    hipLaunchKernelGGL((neptune_mg_line_slow<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, a.q, a.b, a.lo, a.inv, a.up, a.x);
}
template <class T, int MODE>
int line_launch(const MgBox& B, int axis, const LineArgs<T>& a, hipStream_t stream) {
  const LineGrid L = line_grid(B, axis);
  if (axis == 2) {
    if constexpr (MODE == kMgLineFirst)
      hipLaunchKernelGGL(neptune_mg_line_contig_first<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, a.b, a.lo, a.inv, a.up, a.x);
    else if constexpr (MODE == kMgLineDot)
      hipLaunchKernelGGL(neptune_mg_line_contig_dot<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, a.q, a.b, a.lo, a.inv, a.up, a.x, a.partials);
    else
      hipLaunchKernelGGL(neptune_mg_line_contig<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, a.q, a.b, a.lo, a.inv, a.up, a.x);
  } else if (axis == 0) {
    if (L.width == 256) line_slow_launch<T, MODE, 0, 256>(B, L, a, stream);
    else line_slow_launch<T, MODE, 0, 64>(B, L, a, stream);
  } else {
    if (L.width == 256) line_slow_launch<T, MODE, 1, 256>(B, L, a, stream);
    else line_slow_launch<T, MODE, 1, 64>(B, L, a, stream);
  }
  return launched();
}
// mode: kMgLinePlain; kMgLineFirst, the apply-free stage (x from b alone; q is not read); kMgLineDot, the stage that also
// leaves one partial of b . x_new per workgroup of line_grid
int do_line(int dtype, int mode, const MgBox& B, int axis, void* q, const void* b, const void* lo, const void* inv, const void* up, void* x,
            void* partials, hipStream_t s) {
  return by_type(dtype, [&](auto t) {
    using T = decltype(t);
    const LineArgs<T> a = {io<T>(q), in<T>(b), in<T>(lo), in<T>(inv), in<T>(up), io<T>(x), io<T>(partials)};
    if (mode == kMgLineFirst) return line_launch<T, kMgLineFirst>(B, axis, a, s);
    if (mode == kMgLineDot) return line_launch<T, kMgLineDot>(B, axis, a, s);
    return line_launch<T, kMgLinePlain>(B, axis, a, s);
  });
}

int64_t g_mg_counts[3] = {0, 0, 0};   // plain cycles, graph cycles, checks of the last solve

// one solve, its arguments checked
struct Solve {
  const neptune_hip_mg_level_t* levels;
  const neptune_hip_mg_lines_t* lines;   // per level, or nullptr: no level has line stages
  int n_levels, dtype, rank, pre, post, coarse_sweeps;
  MgBox box[kMaxLevels];
  Pair pair[kMaxLevels];                 // pair[l]: levels l and l + 1
  const neptune_hip_launch_cfg_t* cfg;   // level 0's, nullptr unless the caller set anything
  hipStream_t stream;

  // The arguments every solve over a hierarchy shares, checked before anything touches the device, and the solve's fields
  // filled in from them (all but `stream`); -> false: refuse
  bool check(const neptune_hip_mg_level_t* levels_, int n_levels_, int dtype_, int pre_, int post_, int coarse_sweeps_,
             const neptune_hip_launch_cfg_t* cfg_, const neptune_hip_mg_lines_t* lines_ = nullptr,
             const neptune_hip_mg_transfer_t* transfer_ = nullptr, bool symmetric_only = false) {
    if (!levels_ || n_levels_ < 1 || n_levels_ > kMaxLevels || !known_dtype(dtype_)) return false;
    if (pre_ < 0 || post_ < 0 || coarse_sweeps_ < 0) return false;
    levels = levels_;
    lines = lines_;
    n_levels = n_levels_;
    dtype = dtype_;
    pre = pre_;
    post = post_;
    coarse_sweeps = coarse_sweeps_;
    cfg = set_cfg(cfg_);
    rank = levels[0].g.rank;
    const size_t elem = elem_size(dtype);
    for (int l = 0; l < n_levels; ++l) {
      const neptune_hip_mg_level_t& L = levels[l];
      const int n_stages = lines ? lines[l].n_stages : 0;
      if (n_stages < 0 || n_stages > 3) return false;
      if (!L.x || !L.b || !L.q || (!L.minv && n_stages == 0)) return false;   // a level with stages does not read minv
      if (!level_box(&L.g, box[l]) || L.g.rank != rank) return false;
      if (!L.fn) {
        if (L.body < 0 || L.body >= NEPTUNE_HIP_BODY_COUNT) return false;
        if (body_dtype(L.body) != dtype) return false;
      }
      if (L.g.num_inputs > 1 && !L.in_rest) return false;
      for (int i = 1; i < L.g.num_inputs; ++i)
        if (!L.in_rest[i - 1]) return false;
      if (l + 1 < n_levels && !isfinite(L.rscale)) return false;
      if (l > 0) {
        Pair& P = pair[l - 1];
        if (!P.nest(box[l - 1], box[l], rank)) return false;
        if (transfer_ && !P.rules(transfer_[l - 1])) return false;
        if (symmetric_only && P.linear != P.rlinear) return false;   // P must be a multiple of R^T
      }
      const void* mine[4] = {L.x, L.b, L.q, L.minv};
      const size_t bytes = box_bytes(box[l], elem);
      for (int a = 0; a < 4; ++a) {
        if (!mine[a]) continue;   // minv of a level with stages
        if ((uintptr_t)mine[a] % elem != 0) return false;
        for (int o = 0; o < a; ++o)
          if (mine[o] && buffers_overlap(mine[a], bytes, mine[o], bytes)) return false;
        if (l > 0) {
          const neptune_hip_mg_level_t& P = levels[l - 1];
          const void* finer[4] = {P.x, P.b, P.q, P.minv};
          const size_t finer_bytes = box_bytes(box[l - 1], elem);
          for (int o = 0; o < 4; ++o)
            if (finer[o] && buffers_overlap(mine[a], bytes, finer[o], finer_bytes)) return false;
        }
      }
    }
    // the line stages' factor fields: read-only, so they may not meet a field that the level or a neighbour writes
    for (int l = 0; l < n_levels && lines; ++l) {
      const neptune_hip_mg_lines_t& S = lines[l];
      const size_t bytes = box_bytes(box[l], elem);
      for (int s = 0; s < S.n_stages; ++s) {
        if (S.axis[s] < 0 || S.axis[s] >= rank) return false;
        for (const void* f : {S.lo[s], S.inv[s], S.up[s]}) {
          if (!f || (uintptr_t)f % elem != 0) return false;
          for (int o = std::max(l - 1, 0); o <= std::min(l + 1, n_levels - 1); ++o)
            for (const void* w : {(const void*)levels[o].x, (const void*)levels[o].b, (const void*)levels[o].q})
              if (buffers_overlap(f, bytes, w, box_bytes(box[o], elem))) return false;
        }
      }
    }
    return true;
  }
  // every level's factor fields are read while a driver writes `written`: -> false when one meets one of them (one apart()
  // over all of them; `written` itself has passed its own tests in the entry and passes them here once more)
  bool factors_apart(Spans written) const {
    Span factors[kMaxLevels * 9];
    size_t n = 0;
    for (int l = 0; l < n_levels && lines; ++l)
      for (int st = 0; st < lines[l].n_stages; ++st)
        for (const void* f : {lines[l].lo[st], lines[l].inv[st], lines[l].up[st]}) factors[n++] = {f, box_bytes(box[l], elem_size(dtype))};
    return apart(written, Spans(factors, n));
  }
  // x_l = 0 on every level below the finest
  void zero_coarse() const {
    for (int l = 1; l < n_levels; ++l) NEPTUNE_HIP_CHECK(hipMemsetAsync(levels[l].x, 0, box_bytes(box[l], elem_size(dtype)), stream));
  }
  // q_l = A_l(in0), a plain launch
  int apply_of(int l, const void* in0) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    ins[0] = in0;
    for (int i = 1; i < L.g.num_inputs; ++i) ins[i] = L.in_rest[i - 1];
    const neptune_hip_launch_cfg_t* c = l == 0 ? cfg : nullptr;
    return L.fn ? L.fn(&L.g, ins, L.q, (void*)stream, c) : neptune_hip_apply_builtin(L.body, &L.g, ins, L.q, (void*)stream, c);
  }
  // q_l = A_l(x_l)
  int apply(int l) const { return apply_of(l, levels[l].x); }
  int stages(int l) const { return lines ? lines[l].n_stages : 0; }
  // stage `st` of level l without its apply, in the form `mode`
  int line_kernel(int l, int st, int mode, void* partials = nullptr) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const neptune_hip_mg_lines_t& S = lines[l];
    return do_line(dtype, mode, box[l], S.axis[st] + 3 - rank, L.q, L.b, S.lo[st], S.inv[st], S.up[st], L.x, partials, stream);
  }
  // stage `st` of level l: q = A(x), then the line kernel
  int line_stage(int l, int st) const {
    const int rc = apply(l);
    return rc != NEPTUNE_HIP_OK ? rc : line_kernel(l, st, kMgLinePlain);
  }
  // `count` sweeps: the point sweep with minv, or on a level with k >= 1 line stages all k, each after its own apply --
  // stages 0 .. k-1, or k-1 .. 0 when `reversed` (the post-sweeps: a cycle of symmetric stages stays symmetric)
  int sweeps(int l, int count, bool reversed = false) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const int k = stages(l);
    for (int s = 0; s < count; ++s) {
      int rc = NEPTUNE_HIP_OK;
      if (k == 0) {
        rc = apply(l);
        if (rc == NEPTUNE_HIP_OK) rc = do_smooth(dtype, box[l], L.q, L.b, L.minv, L.x, stream);
      }
      for (int t = 0; t < k && rc == NEPTUNE_HIP_OK; ++t) rc = line_stage(l, reversed ? k - 1 - t : t);
      if (rc != NEPTUNE_HIP_OK) return rc;
    }
    return NEPTUNE_HIP_OK;
  }
  // the two transfers of the pair (l, l + 1)
  int restrict_pair(int l) const {
    return do_restrict(dtype, pair[l], levels[l].b, levels[l].q, levels[l].rscale, levels[l + 1].b, levels[l + 1].x, stream);
  }
  int prolong_pair(int l) const { return do_prolong(dtype, pair[l], levels[l + 1].x, levels[l].x, stream); }
  // what a cycle does on level l between its pre- and its post-sweeps: the residual down, the cycle below, the correction up
  int coarse_correction(int l) const {
    int rc = apply(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = restrict_pair(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = cycle(l + 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    return prolong_pair(l);
  }
  int cycle(int l) const {
    if (l == n_levels - 1) return sweeps(l, coarse_sweeps);
    int rc = sweeps(l, pre);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = coarse_correction(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    return sweeps(l, post, true);
  }
  // rr = sum over Omega_0 of (b - A(x))^2 into *rr_dev, then read back: one stream synchronise, one scalar
  int residual(void* rr_dev, double* rr) const {
    int rc = apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = neptune_hip_update_norm(dtype, &levels[0].g, levels[0].b, levels[0].q, rr_dev, (void*)stream);
    if (rc != NEPTUNE_HIP_OK) return rc;
    read_scalars(dtype, stream, rr_dev, 1, rr);
    return NEPTUNE_HIP_OK;
  }
};

bool graph_path_enabled() {
  const char* e = getenv("NEPTUNE_HIP_MG_GRAPH");
  return !(e && strcmp(e, "0") == 0);
}

// ---------------------------------------------------------------- the block loop of every driver
// One unit (a cycle, an iteration) as a graph, this call's: captured on the stream (nothing runs) and instantiated.
struct UnitGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // -> false, and nothing kept: a launch refused under capture, or the runtime would not have the graph
  template <class Unit>
  bool capture(hipStream_t stream, Unit&& unit) {
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int rc = unit();
    if (hipStreamEndCapture(stream, &graph) != hipSuccess) { (void)hipGetLastError(); graph = nullptr; }
    if (rc == NEPTUNE_HIP_OK && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); exec = nullptr; }
    if (exec) return true;
    if (graph) (void)hipGraphDestroy(graph);
    graph = nullptr;
    return false;
  }
  ~UnitGraph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};
// Up to `max` units in blocks of check_every.  The first unit runs as plain launches: it validates the request and lets
// first-use tuning run outside capture.  Then, when at least two more units may follow, ONE capture of unit(); every later
// unit replays that graph, or, when the capture failed, stays a plain unit().  After each block check(&rr) reads rr back (the
// block's one synchronise); the loop ends on rr <= tol2.  A unit or a check that refuses ends the call with late(rc).
// hooks: capturing() before the capture, captured(ok) after it, counted(replayed) after every unit -- the caller's
// counters, and whatever state of its unit a failed capture must not leave changed.
template <class Unit, class Check, class Hooks>
int run_blocks(hipStream_t stream, int64_t max, int64_t check_every, double tol2, int64_t* done_out, double* rr_last, Unit&& unit,
               Check&& check, Hooks&& hooks) {
  UnitGraph G;
  const bool graphs = graph_path_enabled();
  bool tried = false;
  int64_t done = 0;
  while (done < max) {
    const int64_t block = std::min(check_every, max - done);
    for (int64_t c = 0; c < block; ++c, ++done) {
      if (done > 0 && graphs && !tried && max - done >= 2) {
        tried = true;
        hooks.capturing();
        hooks.captured(G.capture(stream, unit));
      }
      if (G.exec) {
        NEPTUNE_HIP_CHECK(hipGraphLaunch(G.exec, stream));
      } else {
        const int rc = unit();
        if (rc != NEPTUNE_HIP_OK) return late(rc);
      }
      hooks.counted(G.exec != nullptr);
      if (done_out) *done_out = done + 1;
    }
    double rr = 0.0;
    const int rc = check(&rr);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    if (rr_last) *rr_last = rr;
    if (rr <= tol2) break;   // false for a NaN: such a solve runs to `max`
  }
  return NEPTUNE_HIP_OK;
}

// ---------------------------------------------------------------- multigrid-preconditioned conjugate gradients
// The device block of the MGCG drivers and the kernel-alone sweeps with a dot product: PcgScalars, then rz_0, then the
// partials of the solver's own kernels; grown on demand, never while a capture is under way.
void* g_mgcg_ws = nullptr;
size_t g_mgcg_ws_bytes = 0;
int64_t g_mgcg_counts[4] = {0, 0, 0, 0};   // plain / graph / fallback iterations, checks of the last mgcg_solve
double g_mgcg_rz0 = 0.0;                   // r . M(r) after the set-up of the last mgcg_solve
constexpr size_t kMgcgRz0Offset = 64;      // room for PcgScalars<double> (56 bytes)
constexpr size_t kMgcgScalarBytes = 80;    // then rz_0; keeps the partials 16-byte aligned
static_assert(sizeof(PcgScalars<double>) <= kMgcgRz0Offset && kMgcgScalarBytes % 16 == 0, "the scalar block");

bool grow_mgcg_ws(size_t bytes, void* stream) {
  if (bytes <= g_mgcg_ws_bytes) return true;
  if (stream_capturing(stream)) return false;
  if (g_mgcg_ws) NEPTUNE_HIP_CHECK(hipFree(g_mgcg_ws));   // waits for every launch that may still use the old block
  g_mgcg_ws = nullptr;
  g_mgcg_ws_bytes = 0;
  NEPTUNE_HIP_CHECK(hipMalloc(&g_mgcg_ws, bytes));
  g_mgcg_ws_bytes = bytes;
  return true;
}
// room for `count` partials of `elem` bytes behind the scalars: -> where they start, nullptr when the block cannot grow now
void* mgcg_partials(int64_t count, size_t elem, void* stream) {
  if (!grow_mgcg_ws(kMgcgScalarBytes + (size_t)count * elem, stream)) return nullptr;
  return static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes;
}

// what an MGCG entry hands its driver once the arguments are checked
struct MgcgArgs {
  neptune_hip_apply_dot_fn fn_dot;
  int sweeps;
  void* const* work;
  int64_t max_iters, check_every;
  double tol2;
  void* trace;
  int64_t* iters_done;
  double* rr0;
  double* rr_last;
};
// The fields of one MGCG solve: conjugate gradients' own in D -- x, b, q of the outer operator, r, p --, level 0 of the
// preconditioner's cycle in S: minv and (z, r_in) for the cycle's (x, b).  scal, partials: the device block.
// lines0: level 0 smooths with line stages.
template <class D, class S>
struct MgcgFields {
  int64_t n;
  D* x;
  const D* b;
  D *q, *r, *p;
  const S* minv;
  S *r_in, *z;
  PcgScalars<D>* scal;
  D* partials;
  bool lines0;
};
// What the two forms of MGCG differ in, a policy each: the element types, whether level 0 may have line stages, the grids of
// the two flat kernels, and four launches -- init (r = b - q, and what the cycle starts from), update (x, r and the cycle's
// start after alpha), direction (p = z + beta p) and p_from_z (the first direction).  Level 0's last post-sweep, the fifth
// launch that differs, is do_smooth_dot with or without the wide sum.
// One type T: r_in is r.  With line stages on level 0, r is stored without z = minv r.
template <class T>
struct MgcgOneType {
  using D = T;
  using S = T;
  using Fields = MgcgFields<T, T>;
  static constexpr bool kLines0 = true;
  static FlatGrid update_grid(const Fields& f) {
    return f.lines0 ? flat_grid(f.n, sizeof(T), {f.p, f.q, f.x, f.r}) : flat_grid(f.n, sizeof(T), {f.p, f.q, f.minv, f.x, f.r, f.z});
  }
  static FlatGrid direction_grid(const Fields& f) { return flat_grid(f.n, sizeof(T), {f.z, f.p}); }
  static void init(const Fields& f, const CgBoxParams& P, int64_t nchunk, dim3 grid, hipStream_t s) {
    if (f.lines0) hipLaunchKernelGGL((neptune_mgcg_init<T, false>), grid, dim3(256), 0, s, P, nchunk, f.b, (const T*)f.q, f.minv, f.r, f.z, f.partials);
    else hipLaunchKernelGGL(neptune_mgcg_init<T>, grid, dim3(256), 0, s, P, nchunk, f.b, (const T*)f.q, f.minv, f.r, f.z, f.partials);
  }
  static void update(const Fields& f, const FlatGrid& g, hipStream_t s) {
    if (f.lines0)
      flat_launch(g, s, neptune_mgcg_update<T, true, false>, neptune_mgcg_update<T, false, false>, f.n, f.scal, f.p, f.q, f.minv, f.x, f.r, f.z, f.partials);
    else flat_launch(g, s, neptune_mgcg_update<T, true>, neptune_mgcg_update<T, false>, f.n, f.scal, f.p, f.q, f.minv, f.x, f.r, f.z, f.partials);
  }
  static void direction(const Fields& f, const FlatGrid& g, hipStream_t s) {
    flat_launch(g, s, neptune_mgcg_direction<T, true>, neptune_mgcg_direction<T, false>, f.n, f.scal, f.z, f.p);
  }
  static void p_from_z(const Fields& f, const FlatGrid&, hipStream_t s) {
    NEPTUNE_HIP_CHECK(hipMemcpyAsync(f.p, f.z, (size_t)f.n * sizeof(T), hipMemcpyDeviceToDevice, s));
  }
};
// Conjugate gradients in f64 around a cycle in f32: r_in = r32, the narrowed residual.  The flat kernels take
// groups of kMixedGroup cells; level 0 has no line stages (a wide-sum form of the line kernels is not built).
struct MgcgMixed {
  using D = double;
  using S = float;
  using Fields = MgcgFields<double, float>;
  static constexpr bool kLines0 = false;
  static FlatGrid update_grid(const Fields& f) { return flat_grid_group(f.n, kMixedGroup, {f.p, f.q, f.minv, f.x, f.r, f.r_in, f.z}); }
  static FlatGrid direction_grid(const Fields& f) { return flat_grid_group(f.n, kMixedGroup, {f.z, f.p}); }
  static void init(const Fields& f, const CgBoxParams& P, int64_t nchunk, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((neptune_mgcg_init_mixed<D, S>), grid, dim3(256), 0, s, P, nchunk, f.b, (const D*)f.q, f.minv, f.r, f.r_in, f.z, f.partials);
  }
  static void update(const Fields& f, const FlatGrid& g, hipStream_t s) {
    flat_launch(g, s, neptune_mgcg_update_mixed<D, S, true>, neptune_mgcg_update_mixed<D, S, false>, f.n, f.scal, f.p, f.q, f.minv, f.x, f.r, f.r_in,
                f.z, f.partials);
  }
  static void direction(const Fields& f, const FlatGrid& g, hipStream_t s) {
    flat_launch(g, s, neptune_mgcg_direction_mixed<D, S, true>, neptune_mgcg_direction_mixed<D, S, false>, f.n, f.scal, f.z, f.p);
  }
  static void p_from_z(const Fields& f, const FlatGrid& g, hipStream_t s) {
    flat_launch(g, s, neptune_mgcg_direction_mixed<D, S, true, true>, neptune_mgcg_direction_mixed<D, S, false, true>, f.n, f.scal, f.z, f.p);
  }
};

// An MGCG solve once its arguments are checked.  S: the solve over the preconditioner's hierarchy, whose level 0 carries
// (z, r_in) for (x, b); O: the outer operator, in D, with the caller's x, b and q (the one-type form: the caller's level 0);
// ocfg: its launch configuration (nullptr unless the caller set anything); a.work = r, p in D.
template <class P>
int mgcg_drive(const Solve& S, const neptune_hip_mg_level_t& O, const neptune_hip_launch_cfg_t* ocfg, const MgcgArgs& a) {
  using D = typename P::D;
  using Sx = typename P::S;
  constexpr int dtype_outer = std::is_same<D, double>::value ? NEPTUNE_HIP_F64 : NEPTUNE_HIP_F32;
  const hipStream_t stream = S.stream;
  const MgBox& B0 = S.box[0];
  const neptune_hip_mg_level_t& F = S.levels[0];
  // k0 >= 1: level 0 smooths with line stages: the cycle starts with the apply-free form of stage 0 and ends
  // with the form of it that yields r . z
  const int k0 = P::kLines0 ? S.stages(0) : 0;
  const int dot_axis = k0 ? S.lines[0].axis[0] + 3 - S.rank : 0;
  typename P::Fields f;
  f.n = B0.n[0] * B0.n[1] * B0.n[2];
  f.x = static_cast<D*>(O.x);
  f.b = static_cast<const D*>(O.b);
  f.q = static_cast<D*>(O.q);
  f.r = static_cast<D*>(a.work[0]);
  f.p = static_cast<D*>(a.work[1]);
  f.minv = static_cast<const Sx*>(F.minv);
  f.r_in = static_cast<Sx*>(F.b);
  f.z = static_cast<Sx*>(F.x);
  f.lines0 = k0 > 0;
  D* const tr = static_cast<D*>(a.trace);

  CgBoxParams Bp;
  for (int d = 0; d < 3; ++d) {
    Bp.n[d] = B0.n[d];
    Bp.lo[d] = B0.lo[d];
    Bp.hi[d] = B0.lo[d] + B0.m[d];
  }
  const int64_t init_chunk = (Bp.n[2] + 255) / 256;
  const dim3 init_grid = grid_for_blocks(Bp.n[0] * Bp.n[1] * init_chunk);
  const FlatGrid upd = P::update_grid(f), dir = P::direction_grid(f);
  const RowGrid sd = row_grid(B0);
  const int64_t dot_blocks = k0 ? grid_blocks(line_grid(B0, dot_axis).grid) : grid_blocks(sd.grid);
  const int64_t most = std::max<int64_t>({grid_blocks(init_grid), (int64_t)upd.blocks, dot_blocks});
  f.partials = static_cast<D*>(mgcg_partials(most, sizeof(D), (void*)stream));   // no capture is under way: the entry refused one
  f.scal = static_cast<PcgScalars<D>*>(g_mgcg_ws);
  D* const rz0_dev = reinterpret_cast<D*>(static_cast<char*>(g_mgcg_ws) + kMgcgRz0Offset);
  auto final_kernel = [&](int64_t count, int stage) {
    hipLaunchKernelGGL(neptune_mgcg_final<D>, dim3(1), dim3(256), 0, stream, (const D*)f.partials, count, f.scal, rz0_dev, tr, a.max_iters, stage);
  };
  // the outer operator: q = A(in0) in D, plainly or through the dot-monitored entry
  const OuterOperator A = {O.fn, a.fn_dot, O.body, &O.g, O.in_rest, ocfg, stream};
  // the rest of M: everything of the cycle on A z = r_in after its first pre-sweep (z = minv r_in, stored with r_in; with
  // line stages: stage 0 without an apply, from z = 0, then the other stages); its last post-sweep yields r_in . z in D,
  // which `stage` of the bookkeeping kernel takes
  auto rest_of_cycle = [&](int stage) -> int {
    int rc = k0 ? S.line_kernel(0, 0, kMgLineFirst) : NEPTUNE_HIP_OK;
    for (int st = 1; st < k0 && rc == NEPTUNE_HIP_OK; ++st) rc = S.line_stage(0, st);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.sweeps(0, a.sweeps - 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.coarse_correction(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.sweeps(0, a.sweeps - 1, true);
    for (int st = k0 - 1; st >= 1 && rc == NEPTUNE_HIP_OK; --st) rc = S.line_stage(0, st);   // the last post-sweep, down to stage 1
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    if (k0) {
      rc = S.line_kernel(0, 0, kMgLineDot, f.partials);
      if (rc != NEPTUNE_HIP_OK) return rc;
    } else {   // the point sweep that yields r_in . z: in D, the wide sum when the cycle's type is narrower
      rc = do_smooth_dot(S.dtype, !std::is_same<D, Sx>::value, B0, F.q, F.b, F.minv, F.x, f.partials, stream);
      if (rc != NEPTUNE_HIP_OK) return rc;
    }
    final_kernel(dot_blocks, stage);
    return launched();
  };

  // ---- set-up
  S.zero_coarse();
  if (!region_is_whole(&O.g)) NEPTUNE_HIP_CHECK(hipMemsetAsync(f.q, 0, (size_t)f.n * sizeof(D), stream));
  // with line stages on level 0, z outside Omega_0 is the error equation's rim: zero-filled here, never written again
  if (k0) NEPTUNE_HIP_CHECK(hipMemsetAsync(f.z, 0, (size_t)f.n * sizeof(Sx), stream));
  int rc = A.apply(f.x, f.q);
  if (rc != NEPTUNE_HIP_OK) return rc;
  P::init(f, Bp, init_chunk, init_grid, stream);
  final_kernel(grid_blocks(init_grid), kMgcgStartRr);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  double rr = 0.0;
  read_scalars(stream, &f.scal->rr, 1, &rr);
  if (done_after_setup(rr, a.tol2, a.max_iters, a.rr0, a.rr_last)) return NEPTUNE_HIP_OK;
  rc = rest_of_cycle(kMgcgStartRz);
  if (rc != NEPTUNE_HIP_OK) return late(rc);
  P::p_from_z(f, dir, stream);

  // ---- one iteration.  fused: q = A(p) and pq out of one dot-monitored launch; a refusal of that entry
  // (NEPTUNE_HIP_EUNSUPPORTED, nothing launched) is remembered: a plain launch and neptune_hip_dot from then on
  bool fused = A.has_dot();
  auto iteration = [&]() -> int {
    int rc;
    if (fused) {
      rc = A.apply_dot(f.p, f.q, &f.scal->pq);
      if (rc == NEPTUNE_HIP_EUNSUPPORTED) fused = false;
      else if (rc != NEPTUNE_HIP_OK) return rc;
    }
    if (!fused) {
      rc = A.apply(f.p, f.q);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      rc = neptune_hip_dot(dtype_outer, &O.g, f.q, f.p, &f.scal->pq, (void*)stream);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
    }
    P::update(f, upd, stream);
    final_kernel((int64_t)upd.blocks, kMgcgRr);
    rc = rest_of_cycle(kMgcgRz);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    P::direction(f, dir, stream);
    return launched();
  };
  // the counters, and `fused` across the capture: what refused under capture may well run outside, so a failed capture
  // restores it; a graph captured without the fused launch counts every replay as a fallback iteration
  struct Hooks {
    bool& fused;
    bool was_fused = false, graph_fallback = false;
    void capturing() { was_fused = fused; }
    void captured(bool ok) {
      if (ok) graph_fallback = !fused;
      else fused = was_fused;
    }
    void counted(bool replayed) {
      ++g_mgcg_counts[replayed ? 1 : 0];
      if (replayed ? graph_fallback : !fused) ++g_mgcg_counts[2];
    }
  } hooks{fused};
  bool rz0_read = false;
  return run_blocks(stream, a.max_iters, a.check_every, a.tol2, a.iters_done, a.rr_last, iteration,
                    [&](double* out) -> int {   // the first check reads rz_0 as well
                      if (!rz0_read) read_scalars(stream, &f.scal->rr, out, (const D*)rz0_dev, &g_mgcg_rz0);
                      else read_scalars(stream, &f.scal->rr, 1, out);
                      rz0_read = true;
                      ++g_mgcg_counts[3];
                      return NEPTUNE_HIP_OK;
                    },
                    hooks);
}

// ---------------------------------------------------------------- the kernel-alone entries' shared parts
// the point sweep with its dot product alone: the sum in `dtype_sum` (dtype itself, or f64 over f32 fields) into *dot_out
int smooth_dot_alone(int dtype, int dtype_sum, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                     void* dot_out, void* stream) {
  if (!q || !b || !minv || !x || !dot_out) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t sum_elem = elem_size(dtype_sum), bytes = box_bytes(B, elem_size(dtype));
  if (!apart({{x, bytes}, {dot_out, sum_elem, sum_elem}}, {{q, bytes}, {b, bytes}, {minv, bytes}})) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const int64_t blocks = grid_blocks(row_grid(B).grid);
  void* const partials = mgcg_partials(blocks, sum_elem, stream);
  if (!partials) return NEPTUNE_HIP_EUNSUPPORTED;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = do_smooth_dot(dtype, dtype_sum != dtype, B, q, b, minv, x, partials, s);
  return rc != NEPTUNE_HIP_OK ? rc : monitor_final(dtype_sum, partials, blocks, dot_out, s);
}
// one line stage alone in the form `mode`: q is null for kMgLineFirst, dot_out for every form but kMgLineDot
int line_alone(int mode, int dtype, const neptune_hip_apply_geom_t* g, int axis, void* q, const void* b, const void* lo, const void* inv,
               const void* up, void* x, void* dot_out, void* stream) {
  const bool dot = mode == kMgLineDot;
  if ((!q && mode != kMgLineFirst) || !b || !lo || !inv || !up || !x || (!dot_out && dot) || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B) || axis < 0 || axis >= g->rank) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype), bytes = box_bytes(B, elem);
  if (!apart({{x, bytes}, {q, bytes, 1, true}, {dot_out, elem, elem, true}}, {{b, bytes}, {lo, bytes}, {inv, bytes}, {up, bytes}}))
    return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const int box_axis = axis + 3 - g->rank;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!dot) return do_line(dtype, mode, B, box_axis, q, b, lo, inv, up, x, nullptr, s);
  const int64_t blocks = grid_blocks(line_grid(B, box_axis).grid);
  void* const partials = mgcg_partials(blocks, elem, stream);
  if (!partials) return NEPTUNE_HIP_EUNSUPPORTED;
  const int rc = do_line(dtype, mode, B, box_axis, q, b, lo, inv, up, x, partials, s);
  return rc != NEPTUNE_HIP_OK ? rc : monitor_final(dtype, partials, blocks, dot_out, s);
}
// a pair's restriction alone; t: the caller's choice, or nullptr: what the pair's grid kind implies
int restrict_alone(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                   const neptune_hip_mg_transfer_t* t, const void* b_fine, const void* q_fine, double rscale, void* b_coarse, void* x_coarse,
                   void* stream) {
  if (!b_fine || !q_fine || !b_coarse || !x_coarse || !known_dtype(dtype) || !isfinite(rscale)) return NEPTUNE_HIP_EINVAL;
  Pair P;
  if (!P.nest(g_fine, g_coarse) || (t && !P.rules(*t))) return NEPTUNE_HIP_EINVAL;
  const size_t fb = box_bytes(P.F, elem_size(dtype)), cb = box_bytes(P.Cb, elem_size(dtype));
  if (!apart({{b_coarse, cb}, {x_coarse, cb}}, {{b_fine, fb}, {q_fine, fb}})) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_restrict(dtype, P, b_fine, q_fine, rscale, b_coarse, x_coarse, reinterpret_cast<hipStream_t>(stream));
}
int prolong_alone(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                  const neptune_hip_mg_transfer_t* t, const void* x_coarse, void* x_fine, void* stream) {
  if (!x_coarse || !x_fine || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  Pair P;
  if (!P.nest(g_fine, g_coarse) || (t && !P.rules(*t))) return NEPTUNE_HIP_EINVAL;
  if (!apart({{x_fine, box_bytes(P.F, elem_size(dtype))}}, {{x_coarse, box_bytes(P.Cb, elem_size(dtype))}})) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_prolong(dtype, P, x_coarse, x_fine, reinterpret_cast<hipStream_t>(stream));
}

// MGCG's own part of what an entry resets before anything is checked
void mgcg_reset() {
  g_mgcg_counts[0] = g_mgcg_counts[1] = g_mgcg_counts[2] = g_mgcg_counts[3] = 0;
  g_mgcg_rz0 = 0.0;
}

}  // namespace

extern "C" {

int neptune_hip_mg_smooth(int dtype, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                          void* stream) {
  if (!q || !b || !minv || !x || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, elem_size(dtype));
  if (!apart({{x, bytes}}, {{q, bytes}, {b, bytes}, {minv, bytes}})) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_smooth(dtype, B, q, b, minv, x, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_smooth_dot(int dtype, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                              void* dot_out, void* stream) {
  if (!known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  return smooth_dot_alone(dtype, dtype, g, q, b, minv, x, dot_out, stream);
}

int neptune_hip_mg_smooth_dot_wide(int dtype, int dtype_sum, const neptune_hip_apply_geom_t* g, const void* q, const void* b,
                                   const void* minv, void* x, void* dot_out, void* stream) {
  if (dtype != NEPTUNE_HIP_F32 || dtype_sum != NEPTUNE_HIP_F64) return NEPTUNE_HIP_EINVAL;
  return smooth_dot_alone(dtype, dtype_sum, g, q, b, minv, x, dot_out, stream);
}

int neptune_hip_mg_line_smooth(int dtype, const neptune_hip_apply_geom_t* g, int axis, void* q, const void* b, const void* lo,
                               const void* inv, const void* up, void* x, void* stream) {
  return line_alone(kMgLinePlain, dtype, g, axis, q, b, lo, inv, up, x, nullptr, stream);
}

int neptune_hip_mg_line_first(int dtype, const neptune_hip_apply_geom_t* g, int axis, const void* b, const void* lo, const void* inv,
                              const void* up, void* x, void* stream) {
  return line_alone(kMgLineFirst, dtype, g, axis, nullptr, b, lo, inv, up, x, nullptr, stream);
}

int neptune_hip_mg_line_smooth_dot(int dtype, const neptune_hip_apply_geom_t* g, int axis, void* q, const void* b, const void* lo,
                                   const void* inv, const void* up, void* x, void* dot_out, void* stream) {
  return line_alone(kMgLineDot, dtype, g, axis, q, b, lo, inv, up, x, dot_out, stream);
}

int neptune_hip_mg_restrict(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                            const void* b_fine, const void* q_fine, double rscale, void* b_coarse, void* x_coarse, void* stream) {
  return restrict_alone(dtype, g_fine, g_coarse, nullptr, b_fine, q_fine, rscale, b_coarse, x_coarse, stream);
}

int neptune_hip_mg_restrict_linear(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                                   const neptune_hip_mg_transfer_t* t, const void* b_fine, const void* q_fine, double rscale, void* b_coarse,
                                   void* x_coarse, void* stream) {
  if (!t) return NEPTUNE_HIP_EINVAL;
  return restrict_alone(dtype, g_fine, g_coarse, t, b_fine, q_fine, rscale, b_coarse, x_coarse, stream);
}

int neptune_hip_mg_prolong_add(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                               const void* x_coarse, void* x_fine, void* stream) {
  return prolong_alone(dtype, g_fine, g_coarse, nullptr, x_coarse, x_fine, stream);
}

int neptune_hip_mg_prolong_add_linear(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                                      const neptune_hip_mg_prolong_t* p, const void* x_coarse, void* x_fine, void* stream) {
  if (!p) return NEPTUNE_HIP_EINVAL;
  const neptune_hip_mg_transfer_t t = transfer_of(*p);
  return prolong_alone(dtype, g_fine, g_coarse, &t, x_coarse, x_fine, stream);
}

int neptune_hip_mg_coarsened_axes(const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse, int* mask_out) {
  Pair P;
  if (!mask_out || !P.nest(g_fine, g_coarse)) return NEPTUNE_HIP_EINVAL;
  *mask_out = (P.mask & 7) >> (3 - P.rank);   // the kernels' axes are the dimensions right-aligned
  return NEPTUNE_HIP_OK;
}

int neptune_hip_mg_halved_axes(const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse, int* mask_out) {
  Pair P;
  if (!mask_out || !P.nest(g_fine, g_coarse)) return NEPTUNE_HIP_EINVAL;
  *mask_out = (P.mask & kMgCell) ? (P.mask & 7) >> (3 - P.rank) : 0;
  return NEPTUNE_HIP_OK;
}

void neptune_hip_mg_counts(int64_t* plain_cycles, int64_t* graph_cycles, int64_t* checks) {
  if (plain_cycles) *plain_cycles = g_mg_counts[0];
  if (graph_cycles) *graph_cycles = g_mg_counts[1];
  if (checks) *checks = g_mg_counts[2];
}

int neptune_hip_mg_solve(const neptune_hip_mg_level_t* levels, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                         int64_t max_cycles, int64_t check_every, double tol2, double* rr_checks, void* stream,
                         const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done, double* rr0, double* rr_last) {
  return neptune_hip_mg_solve_lines(levels, nullptr, n_levels, dtype, pre, post, coarse_sweeps, max_cycles, check_every, tol2, rr_checks,
                                    stream, cfg, cycles_done, rr0, rr_last);
}

int neptune_hip_mg_solve_lines(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines, int n_levels, int dtype,
                               int pre, int post, int coarse_sweeps, int64_t max_cycles, int64_t check_every, double tol2,
                               double* rr_checks, void* stream, const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done,
                               double* rr0, double* rr_last) {
  return neptune_hip_mg_solve_prolong(levels, lines, nullptr, n_levels, dtype, pre, post, coarse_sweeps, max_cycles, check_every, tol2,
                                      rr_checks, stream, cfg, cycles_done, rr0, rr_last);
}

int neptune_hip_mg_solve_prolong(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines,
                                 const neptune_hip_mg_prolong_t* prolong, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                                 int64_t max_cycles, int64_t check_every, double tol2, double* rr_checks, void* stream,
                                 const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done, double* rr0, double* rr_last) {
  // the same choice per pair with the averaging restriction; an n_levels out of range is refused below whatever the array
  neptune_hip_mg_transfer_t tr[kMaxLevels];
  const bool have = prolong && n_levels >= 1 && n_levels <= kMaxLevels;
  for (int l = 0; have && l + 1 < n_levels; ++l) tr[l] = transfer_of(prolong[l]);
  return neptune_hip_mg_solve_transfer(levels, lines, have ? tr : nullptr, n_levels, dtype, pre, post, coarse_sweeps, max_cycles, check_every,
                                       tol2, rr_checks, stream, cfg, cycles_done, rr0, rr_last);
}

int neptune_hip_mg_solve_transfer(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines,
                                  const neptune_hip_mg_transfer_t* transfer, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                                  int64_t max_cycles, int64_t check_every, double tol2, double* rr_checks, void* stream,
                                  const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done, double* rr0, double* rr_last) {
  g_mg_counts[0] = g_mg_counts[1] = g_mg_counts[2] = 0;
  reset_solver_outputs(cycles_done, rr0, rr_last);
  // ---- the refusals, before anything touches the device
  if (check_every < 1 || max_cycles < 0) return NEPTUNE_HIP_EINVAL;
  Solve S;
  if (!S.check(levels, n_levels, dtype, pre, post, coarse_sweeps, cfg, lines, transfer)) return NEPTUNE_HIP_EINVAL;
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  struct Scalar {   // one device T for r . r, this call's
    void* p = nullptr;
    Scalar() { NEPTUNE_HIP_CHECK(hipMalloc(&p, 8)); }
    ~Scalar() { (void)hipFree(p); }
  } rr_dev;

  S.zero_coarse();
  double rr = 0.0;
  const int rc = S.residual(rr_dev.p, &rr);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (done_after_setup(rr, tol2, max_cycles, rr0, rr_last)) return NEPTUNE_HIP_OK;

  struct Hooks {
    void capturing() {}
    void captured(bool) {}
    void counted(bool replayed) { ++g_mg_counts[replayed ? 1 : 0]; }
  };
  return run_blocks(S.stream, max_cycles, check_every, tol2, cycles_done, rr_last, [&] { return S.cycle(0); },
                    [&](double* out) -> int {
                      const int rc = S.residual(rr_dev.p, out);
                      if (rc != NEPTUNE_HIP_OK) return rc;
                      if (rr_checks) rr_checks[g_mg_counts[2]] = *out;
                      ++g_mg_counts[2];
                      return NEPTUNE_HIP_OK;
                    },
                    Hooks());
}

int neptune_hip_mgcg_solve_mixed(const neptune_hip_mg_level_t* outer, int dtype_outer, neptune_hip_apply_dot_fn fn_dot,
                                 const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines, int n_levels, int dtype_inner,
                                 int sweeps, int coarse_sweeps, void* const work[2], int64_t max_iters, int64_t check_every, double tol2,
                                 void* trace, void* stream, const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0,
                                 double* rr_last) {
  return neptune_hip_mgcg_solve_mixed_transfer(outer, dtype_outer, fn_dot, levels, lines, nullptr, n_levels, dtype_inner, sweeps, coarse_sweeps,
                                               work, max_iters, check_every, tol2, trace, stream, cfg, iters_done, rr0, rr_last);
}

int neptune_hip_mgcg_solve_mixed_transfer(const neptune_hip_mg_level_t* outer, int dtype_outer, neptune_hip_apply_dot_fn fn_dot,
                                          const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines,
                                          const neptune_hip_mg_transfer_t* transfer, int n_levels, int dtype_inner, int sweeps,
                                          int coarse_sweeps, void* const work[2], int64_t max_iters, int64_t check_every, double tol2,
                                          void* trace, void* stream, const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0,
                                          double* rr_last) {
  mgcg_reset();
  reset_solver_outputs(iters_done, rr0, rr_last);
  // ---- the refusals, before anything touches the device
  if (dtype_outer != NEPTUNE_HIP_F64 || dtype_inner != NEPTUNE_HIP_F32) return NEPTUNE_HIP_EINVAL;
  if (!outer || n_levels < 2 || sweeps < 1 || check_every < 1 || max_iters < 0 || !work) return NEPTUNE_HIP_EINVAL;
  Solve S;   // the inner hierarchy; cfg belongs to the outer operator
  if (!S.check(levels, n_levels, dtype_inner, sweeps, sweeps, coarse_sweeps, nullptr, lines, transfer, true)) return NEPTUNE_HIP_EINVAL;
  // the outer operator: what Solve::check asks of a level's operator, in D, and level 0's box and Omega
  const neptune_hip_mg_level_t& O = *outer;
  MgBox OB;
  if (!O.x || !O.b || !O.q || !level_box(&O.g, OB) || O.g.rank != S.rank) return NEPTUNE_HIP_EINVAL;
  for (int a = 0; a < 3; ++a)
    if (OB.n[a] != S.box[0].n[a] || OB.lo[a] != S.box[0].lo[a] || OB.m[a] != S.box[0].m[a]) return NEPTUNE_HIP_EINVAL;
  if (!O.fn && (O.body < 0 || O.body >= NEPTUNE_HIP_BODY_COUNT || O.body == NEPTUNE_HIP_BODY_LAP3D27_F32)) return NEPTUNE_HIP_EINVAL;
  if (O.g.num_inputs > 1 && !O.in_rest) return NEPTUNE_HIP_EINVAL;
  for (int i = 1; i < O.g.num_inputs; ++i)
    if (!O.in_rest[i - 1]) return NEPTUNE_HIP_EINVAL;
  // the wide fields and the trace may meet neither each other nor an inner field of levels 0 and 1 (each inner level's own
  // four were checked against each other and the neighbour's above); minv of a level with line stages may be null
  const size_t wide0 = box_bytes(OB, sizeof(double)), narrow0 = box_bytes(S.box[0], sizeof(float)), narrow1 = box_bytes(S.box[1], sizeof(float));
  const Span wide[6] = {{O.x, wide0, 8},     {O.b, wide0, 8},     {O.q, wide0, 8},
                        {work[0], wide0, 8}, {work[1], wide0, 8}, {trace, (size_t)(3 * max_iters) * sizeof(double), 8, true}};
  if (!apart(wide, {{levels[0].x, narrow0, 4}, {levels[0].b, narrow0, 4}, {levels[0].q, narrow0, 4}, {levels[0].minv, narrow0, 4, true},
                    {levels[1].x, narrow1, 4}, {levels[1].b, narrow1, 4}, {levels[1].q, narrow1, 4}, {levels[1].minv, narrow1, 4, true}}))
    return NEPTUNE_HIP_EINVAL;
  // line stages on level 0 need a wide-sum form of both code paths of the line kernel: not built yet
  if (S.stages(0) > 0) return NEPTUNE_HIP_EUNSUPPORTED;
  // the factor fields are read while x, q, r, p and the trace are written
  if (!S.factors_apart(wide)) return NEPTUNE_HIP_EINVAL;
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  const MgcgArgs a = {fn_dot, sweeps, work, max_iters, check_every, tol2, trace, iters_done, rr0, rr_last};
  return mgcg_drive<MgcgMixed>(S, O, set_cfg(cfg), a);
}

double neptune_hip_mgcg_rz0(void) { return g_mgcg_rz0; }

void neptune_hip_mgcg_counts(int64_t* plain_iters, int64_t* graph_iters, int64_t* fallback_iters, int64_t* checks) {
  if (plain_iters) *plain_iters = g_mgcg_counts[0];
  if (graph_iters) *graph_iters = g_mgcg_counts[1];
  if (fallback_iters) *fallback_iters = g_mgcg_counts[2];
  if (checks) *checks = g_mgcg_counts[3];
}

int neptune_hip_mgcg_solve(const neptune_hip_mg_level_t* levels, int n_levels, int dtype, neptune_hip_apply_dot_fn fn_dot, int sweeps,
                           int coarse_sweeps, void* const work[3], int64_t max_iters, int64_t check_every, double tol2, void* trace,
                           void* stream, const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0, double* rr_last) {
  return neptune_hip_mgcg_solve_lines(levels, nullptr, n_levels, dtype, fn_dot, sweeps, coarse_sweeps, work, max_iters, check_every, tol2,
                                      trace, stream, cfg, iters_done, rr0, rr_last);
}

int neptune_hip_mgcg_solve_lines(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines, int n_levels, int dtype,
                                 neptune_hip_apply_dot_fn fn_dot, int sweeps, int coarse_sweeps, void* const work[3], int64_t max_iters,
                                 int64_t check_every, double tol2, void* trace, void* stream, const neptune_hip_launch_cfg_t* cfg,
                                 int64_t* iters_done, double* rr0, double* rr_last) {
  return neptune_hip_mgcg_solve_transfer(levels, lines, nullptr, n_levels, dtype, fn_dot, sweeps, coarse_sweeps, work, max_iters, check_every,
                                         tol2, trace, stream, cfg, iters_done, rr0, rr_last);
}

int neptune_hip_mgcg_solve_transfer(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines,
                                    const neptune_hip_mg_transfer_t* transfer, int n_levels, int dtype, neptune_hip_apply_dot_fn fn_dot,
                                    int sweeps, int coarse_sweeps, void* const work[3], int64_t max_iters, int64_t check_every, double tol2,
                                    void* trace, void* stream, const neptune_hip_launch_cfg_t* cfg, int64_t* iters_done, double* rr0,
                                    double* rr_last) {
  mgcg_reset();
  reset_solver_outputs(iters_done, rr0, rr_last);
  // ---- the refusals, before anything touches the device
  if (n_levels < 2 || sweeps < 1 || check_every < 1 || max_iters < 0 || !work) return NEPTUNE_HIP_EINVAL;
  Solve S;
  if (!S.check(levels, n_levels, dtype, sweeps, sweeps, coarse_sweeps, cfg, lines, transfer, true)) return NEPTUNE_HIP_EINVAL;
  // r, p, z and the trace may meet neither each other nor a field of levels 0 and 1; minv of a level with stages may be null
  const size_t elem = elem_size(dtype), bytes0 = box_bytes(S.box[0], elem), bytes1 = box_bytes(S.box[1], elem);
  const Span own[4] = {{work[0], bytes0, elem}, {work[1], bytes0, elem}, {work[2], bytes0, elem}, {trace, (size_t)(3 * max_iters) * elem, elem, true}};
  if (!apart(own, {{levels[0].x, bytes0}, {levels[0].b, bytes0}, {levels[0].q, bytes0}, {levels[0].minv, bytes0, 1, true},
                   {levels[1].x, bytes1}, {levels[1].b, bytes1}, {levels[1].q, bytes1}, {levels[1].minv, bytes1, 1, true}}))
    return NEPTUNE_HIP_EINVAL;
  // the factor fields are read while r, p, z and the trace are written
  if (!S.factors_apart(own)) return NEPTUNE_HIP_EINVAL;
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  StreamScope sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  // the preconditioner's hierarchy: level 0 carries (z, r) for (x, b)
  neptune_hip_mg_level_t lv[kMaxLevels];
  for (int l = 0; l < n_levels; ++l) lv[l] = levels[l];
  lv[0].x = work[2];
  lv[0].b = work[0];
  S.levels = lv;
  const MgcgArgs a = {fn_dot, sweeps, work, max_iters, check_every, tol2, trace, iters_done, rr0, rr_last};
  return by_type(dtype, [&](auto t) { return mgcg_drive<MgcgOneType<decltype(t)>>(S, levels[0], S.cfg, a); });
}

}  // extern "C"
