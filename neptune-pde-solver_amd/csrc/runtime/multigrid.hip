// multigrid.hip -- include/neptune_hip.h: geometric multigrid V-cycles over a hierarchy of applies.
// neptune_hip_mg_smooth / _restrict / _prolong_add launch the three kernels of multigrid_kernels.hpp alone;
// neptune_hip_mg_solve is the cycle driver: the levels' operators through the public C API, the kernels in between, r . r
// through neptune_hip_update_norm, and its own small capture / replay of ONE cycle (a linear graph on the call's stream,
// captured once per call, destroyed when the call returns).  Its own translation unit (builds in seconds, linked into
// libneptune_hip.so): host code plus the kernels' instantiations.  neptune_hip_mg_line_smooth launches one stage of the line
// smoother (mg_line_kernels.hpp) alone; neptune_hip_mg_solve_lines is the driver with line stages per level, and
// neptune_hip_mg_solve is that call without any.  neptune_hip_mgcg_solve_lines is multigrid-preconditioned CG with line stages
// (DESIGN 3.18): on level 0 the cycle starts with the apply-free form of the stage and ends with the form that yields r . z
// (neptune_hip_mg_line_first, neptune_hip_mg_line_smooth_dot launch the two alone); neptune_hip_mgcg_solve is that call without
// lines.  neptune_hip_mgcg_solve_mixed is that solver with x, b, r, p, q and the scalars in f64 around the cycle in f32
// (mgcg_mixed_kernels.hpp); neptune_hip_mg_smooth_dot_wide launches its last sweep, the one with the wide sum, alone.
// A pair of levels is vertex-centred or cell-centred: sizes_nest infers which, and the two transfer launches
// dispatch on it -- everything else here is the same code for both.  A cell-centred pair may prolong linearly instead, by a rule
// per face that the caller states: neptune_hip_mg_prolong_add_linear launches that kernel alone,
// neptune_hip_mg_solve_prolong is the plain-cycle driver with the choice per pair, and neptune_hip_mg_solve_lines is that call
// without any.  The restriction of such a pair may be the transpose of that prolongation: one
// neptune_hip_mg_transfer_t per pair states both transfers and the one rule array they share; neptune_hip_mg_restrict_linear
// launches that kernel alone, neptune_hip_mg_solve_transfer is the plain-cycle driver (neptune_hip_mg_solve_prolong is that
// call with the averaging restriction everywhere), and the neptune_hip_mgcg_*_transfer drivers take a pair only when it is
// symmetric -- CONSTANT with AVERAGE, or LINEAR with LINEAR; the older MGCG entries are those calls without an array.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "../../../include/neptune_hip.h"
#include "../kernels/apply_launch.hpp"   // NEPTUNE_HIP_CHECK, geom_validate, buffers_overlap (no apply kernel is instantiated here)
#include "../kernels/multigrid_kernels.hpp"
#include "../kernels/mg_line_kernels.hpp"
#include "../kernels/mgcg_kernels.hpp"
#include "../kernels/mgcg_mixed_kernels.hpp"

using namespace neptune_hip;

namespace {

constexpr int kMaxLevels = 16;

// what neptune_hip_rt.hip's ensure_init does (device 0 unless the runtime is up already), through the public API
void ensure_init() { (void)neptune_hip_cu_count(); }

bool known_dtype(int dtype) { return dtype == NEPTUNE_HIP_F64 || dtype == NEPTUNE_HIP_F32; }
size_t elem_size(int dtype) { return dtype == NEPTUNE_HIP_F64 ? 8 : 4; }

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
size_t box_bytes(const MgBox& B, size_t elem) { return (size_t)(B.n[0] * B.n[1] * B.n[2]) * elem; }

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

int launched() { return hipGetLastError() == hipSuccess ? NEPTUNE_HIP_OK : NEPTUNE_HIP_EUNSUPPORTED; }

template <class T>
int smooth_launch(const MgBox& B, const void* q, const void* b, const void* minv, void* x, hipStream_t stream) {
  const RowGrid r = row_grid(B);
  hipLaunchKernelGGL(neptune_mg_smooth<T>, r.grid, dim3(256), 0, stream, B, r.nchunk, static_cast<const T*>(q), static_cast<const T*>(b),
                     static_cast<const T*>(minv), static_cast<T*>(x));
  return launched();
}
template <class T, int MASK>
int restrict_launch(const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c, void* x_c,
                    hipStream_t stream) {
  const RowGrid r = row_grid(Cb);
  // axis 2 coarsened: the fine row segments staged in LDS; kept: every lane on its own fine cells
  if constexpr ((MASK & 4) != 0)
    hipLaunchKernelGGL((neptune_mg_restrict<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(b_f),
                       static_cast<const T*>(q_f), (T)rscale, static_cast<T*>(b_c), static_cast<T*>(x_c));
  else
    hipLaunchKernelGGL((neptune_mg_restrict_kept2<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(b_f),
                       static_cast<const T*>(q_f), (T)rscale, static_cast<T*>(b_c), static_cast<T*>(x_c));
  return launched();
}
template <class T, int MASK>
int prolong_launch(const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t stream) {
  const RowGrid r = row_grid(F);
  hipLaunchKernelGGL((neptune_mg_prolong_add<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(x_c),
                     static_cast<T*>(x_f));
  return launched();
}
// the transfers of a cell-centred pair: MASK = the halved axes
template <class T, int MASK>
int restrict_cell_launch(const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c, void* x_c,
                         hipStream_t stream) {
  const RowGrid r = row_grid(Cb);
  hipLaunchKernelGGL((neptune_mg_restrict_cell<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(b_f),
                     static_cast<const T*>(q_f), (T)rscale, static_cast<T*>(b_c), static_cast<T*>(x_c));
  return launched();
}
template <class T, int MASK>
int prolong_cell_launch(const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t stream) {
  const RowGrid r = row_grid(F);
  hipLaunchKernelGGL((neptune_mg_prolong_add_cell<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, static_cast<const T*>(x_c),
                     static_cast<T*>(x_f));
  return launched();
}
// The linear prolongation of a cell-centred pair: one workgroup per chunk of a fine row -- 256 COARSE cells
// (512 fine ones) where axis 2 is halved, 256 fine cells where it is kept
template <class T, int MASK>
int prolong_linear_launch(const MgBox& F, const MgBox& Cb, const MgRim& rim, const void* x_c, void* x_f, hipStream_t stream) {
  RowGrid r;
  r.nchunk = (Cb.m[2] + 255) / 256;   // axis 2 kept: Cb.m[2] = F.m[2]
  r.grid = grid_for_blocks(F.m[0] * F.m[1] * r.nchunk);
  hipLaunchKernelGGL((neptune_mg_prolong_add_linear<T, MASK>), r.grid, dim3(256), 0, stream, F, Cb, r.nchunk, rim, static_cast<const T*>(x_c),
                     static_cast<T*>(x_f));
  return launched();
}
// The transposed linear restriction of a cell-centred pair: one workgroup per 256-cell chunk of a run of
// kMgLinearRun coarse rows of one coarse plane
template <class T, int MASK>
int restrict_linear_launch(const MgBox& F, const MgBox& Cb, const MgRim& rim, const void* b_f, const void* q_f, double rscale, void* b_c,
                           void* x_c, hipStream_t stream) {
  const int64_t nchunk = (Cb.m[2] + 255) / 256, nrun = (Cb.m[1] + kMgLinearRun - 1) / kMgLinearRun;
  hipLaunchKernelGGL((neptune_mg_restrict_linear<T, MASK>), grid_for_blocks(Cb.m[0] * nrun * nchunk), dim3(256), 0, stream, F, Cb, nchunk, rim,
                     static_cast<const T*>(b_f), static_cast<const T*>(q_f), (T)rscale, static_cast<T*>(b_c), static_cast<T*>(x_c));
  return launched();
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
// q: unused by kMgLineFirst; partials: one T per workgroup of the grid, kMgLineDot only
template <class T, int MODE, int AXIS, int WIDTH>
void line_slow_launch(const MgBox& B, const LineGrid& L, void* q, const void* b, const void* lo, const void* inv, const void* up, void* x,
                      void* partials, hipStream_t stream) {
  const T *bp = static_cast<const T*>(b), *lp = static_cast<const T*>(lo), *ip = static_cast<const T*>(inv), *up_ = static_cast<const T*>(up);
  if constexpr (MODE == kMgLineFirst)
    hipLaunchKernelGGL((neptune_mg_line_slow_first<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, bp, lp, ip, up_, static_cast<T*>(x));
  else if constexpr (MODE == kMgLineDot)
    hipLaunchKernelGGL((neptune_mg_line_slow_dot<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, static_cast<T*>(q), bp, lp, ip,
                       up_, static_cast<T*>(x), static_cast<T*>(partials));
  else
    hipLaunchKernelGGL((neptune_mg_line_slow<T, AXIS, WIDTH>), L.grid, dim3(WIDTH), 0, stream, B, L.nchunk, static_cast<T*>(q), bp, lp, ip, up_,
                       static_cast<T*>(x));
}
template <class T, int MODE>
int line_launch(const MgBox& B, int axis, void* q, const void* b, const void* lo, const void* inv, const void* up, void* x, void* partials,
                hipStream_t stream) {
  const LineGrid L = line_grid(B, axis);
  if (axis == 2) {
    const T *bp = static_cast<const T*>(b), *lp = static_cast<const T*>(lo), *ip = static_cast<const T*>(inv), *up_ = static_cast<const T*>(up);
    if constexpr (MODE == kMgLineFirst)
      hipLaunchKernelGGL(neptune_mg_line_contig_first<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, bp, lp, ip, up_, static_cast<T*>(x));
    else if constexpr (MODE == kMgLineDot)
      hipLaunchKernelGGL(neptune_mg_line_contig_dot<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, static_cast<T*>(q), bp, lp, ip, up_,
                         static_cast<T*>(x), static_cast<T*>(partials));
    else
      hipLaunchKernelGGL(neptune_mg_line_contig<T>, L.grid, dim3(kMgLineGroup), 0, stream, B, static_cast<T*>(q), bp, lp, ip, up_,
                         static_cast<T*>(x));
    return launched();
  }
  if (axis == 0) {
    if (L.width == 256) line_slow_launch<T, MODE, 0, 256>(B, L, q, b, lo, inv, up, x, partials, stream);
    else line_slow_launch<T, MODE, 0, 64>(B, L, q, b, lo, inv, up, x, partials, stream);
  } else {
    if (L.width == 256) line_slow_launch<T, MODE, 1, 256>(B, L, q, b, lo, inv, up, x, partials, stream);
    else line_slow_launch<T, MODE, 1, 64>(B, L, q, b, lo, inv, up, x, partials, stream);
  }
  return launched();
}
// the dispatch on element type and on the pair's mask (sizes_nest: the axes 1..7, kMgCell for a cell-centred pair), stated once
template <class F64, class F32>
int by_type(int dtype, F64&& f64, F32&& f32) { return dtype == NEPTUNE_HIP_F64 ? f64() : f32(); }
int do_line(int dtype, const MgBox& B, int axis, void* q, const void* b, const void* lo, const void* inv, const void* up, void* x,
            hipStream_t s) {
  return by_type(dtype, [&] { return line_launch<double, kMgLinePlain>(B, axis, q, b, lo, inv, up, x, nullptr, s); },
                 [&] { return line_launch<float, kMgLinePlain>(B, axis, q, b, lo, inv, up, x, nullptr, s); });
}
// the apply-free stage (x from b alone) and the stage that also leaves one partial of b . x_new per workgroup of line_grid
int do_line_first(int dtype, const MgBox& B, int axis, const void* b, const void* lo, const void* inv, const void* up, void* x, hipStream_t s) {
  return by_type(dtype, [&] { return line_launch<double, kMgLineFirst>(B, axis, nullptr, b, lo, inv, up, x, nullptr, s); },
                 [&] { return line_launch<float, kMgLineFirst>(B, axis, nullptr, b, lo, inv, up, x, nullptr, s); });
}
int do_line_dot(int dtype, const MgBox& B, int axis, void* q, const void* b, const void* lo, const void* inv, const void* up, void* x,
                void* partials, hipStream_t s) {
  return by_type(dtype, [&] { return line_launch<double, kMgLineDot>(B, axis, q, b, lo, inv, up, x, partials, s); },
                 [&] { return line_launch<float, kMgLineDot>(B, axis, q, b, lo, inv, up, x, partials, s); });
}
int do_smooth(int dtype, const MgBox& B, const void* q, const void* b, const void* minv, void* x, hipStream_t s) {
  return by_type(dtype, [&] { return smooth_launch<double>(B, q, b, minv, x, s); }, [&] { return smooth_launch<float>(B, q, b, minv, x, s); });
}
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
int do_restrict(int dtype, int mask, const MgBox& F, const MgBox& Cb, const void* b_f, const void* q_f, double rscale, void* b_c,
                void* x_c, hipStream_t s) {
  return by_mask(mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    if (mask & kMgCell)
      return by_type(dtype, [&] { return restrict_cell_launch<double, M>(F, Cb, b_f, q_f, rscale, b_c, x_c, s); },
                     [&] { return restrict_cell_launch<float, M>(F, Cb, b_f, q_f, rscale, b_c, x_c, s); });
    return by_type(dtype, [&] { return restrict_launch<double, M>(F, Cb, b_f, q_f, rscale, b_c, x_c, s); },
                   [&] { return restrict_launch<float, M>(F, Cb, b_f, q_f, rscale, b_c, x_c, s); });
  });
}
int do_prolong(int dtype, int mask, const MgBox& F, const MgBox& Cb, const void* x_c, void* x_f, hipStream_t s) {
  return by_mask(mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    if (mask & kMgCell)
      return by_type(dtype, [&] { return prolong_cell_launch<double, M>(F, Cb, x_c, x_f, s); },
                     [&] { return prolong_cell_launch<float, M>(F, Cb, x_c, x_f, s); });
    return by_type(dtype, [&] { return prolong_launch<double, M>(F, Cb, x_c, x_f, s); },
                   [&] { return prolong_launch<float, M>(F, Cb, x_c, x_f, s); });
  });
}
int do_prolong_linear(int dtype, int mask, const MgBox& F, const MgBox& Cb, const MgRim& rim, const void* x_c, void* x_f, hipStream_t s) {
  return by_mask(mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    return by_type(dtype, [&] { return prolong_linear_launch<double, M>(F, Cb, rim, x_c, x_f, s); },
                   [&] { return prolong_linear_launch<float, M>(F, Cb, rim, x_c, x_f, s); });
  });
}
int do_restrict_linear(int dtype, int mask, const MgBox& F, const MgBox& Cb, const MgRim& rim, const void* b_f, const void* q_f, double rscale,
                       void* b_c, void* x_c, hipStream_t s) {
  return by_mask(mask & 7, [&](auto m) {
    constexpr int M = decltype(m)::value;
    return by_type(dtype, [&] { return restrict_linear_launch<double, M>(F, Cb, rim, b_f, q_f, rscale, b_c, x_c, s); },
                   [&] { return restrict_linear_launch<float, M>(F, Cb, rim, b_f, q_f, rscale, b_c, x_c, s); });
  });
}
// What the caller states about the prolongation of one pair (sizes_nest's `mask`): -> false: refuse -- a kind outside
// {CONSTANT, LINEAR}, LINEAR on a pair without a halved dimension, a rule outside {EVEN, ODD} on a dimension < rank of a
// LINEAR pair.  *linear: the kind; rim: a LINEAR pair's rules on the kernels' axes (the dimensions right-aligned).
// Nothing but `kind` is read of a CONSTANT entry, and no entry of a dimension >= rank.
bool prolong_rules(const neptune_hip_mg_prolong_t& p, int mask, int rank, bool* linear, MgRim& rim) {
  if (p.kind != NEPTUNE_HIP_MG_PROLONG_CONSTANT && p.kind != NEPTUNE_HIP_MG_PROLONG_LINEAR) return false;
  *linear = p.kind == NEPTUNE_HIP_MG_PROLONG_LINEAR;
  for (int a = 0; a < 3; ++a) rim.lo[a] = rim.hi[a] = NEPTUNE_HIP_MG_RIM_EVEN;
  if (!*linear) return true;
  if (!(mask & kMgCell)) return false;
  for (int d = 0; d < rank; ++d) {
    for (const int32_t v : {p.rim_lo[d], p.rim_hi[d]})
      if (v != NEPTUNE_HIP_MG_RIM_EVEN && v != NEPTUNE_HIP_MG_RIM_ODD) return false;
    rim.lo[d + 3 - rank] = p.rim_lo[d];
    rim.hi[d + 3 - rank] = p.rim_hi[d];
  }
  return true;
}

// The same for both transfers of one pair: -> false: refuse -- what prolong_rules refuses of t.prolong, a
// restrict_kind outside {AVERAGE, LINEAR}, LINEAR restriction on a pair without a halved dimension, a rule outside {EVEN,
// ODD} on a dimension < rank when either transfer is LINEAR.  The one rule array serves both.  Nothing but the two kinds is
// read of a CONSTANT / AVERAGE entry.
bool transfer_rules(const neptune_hip_mg_transfer_t& t, int mask, int rank, bool* linear, bool* rlinear, MgRim& rim) {
  if (t.prolong != NEPTUNE_HIP_MG_PROLONG_CONSTANT && t.prolong != NEPTUNE_HIP_MG_PROLONG_LINEAR) return false;
  if (t.restrict_kind != NEPTUNE_HIP_MG_RESTRICT_AVERAGE && t.restrict_kind != NEPTUNE_HIP_MG_RESTRICT_LINEAR) return false;
  *linear = t.prolong == NEPTUNE_HIP_MG_PROLONG_LINEAR;
  *rlinear = t.restrict_kind == NEPTUNE_HIP_MG_RESTRICT_LINEAR;
  neptune_hip_mg_prolong_t p;
  p.kind = (*linear || *rlinear) ? NEPTUNE_HIP_MG_PROLONG_LINEAR : NEPTUNE_HIP_MG_PROLONG_CONSTANT;
  for (int d = 0; d < 3; ++d) {
    p.rim_lo[d] = t.rim_lo[d];
    p.rim_hi[d] = t.rim_hi[d];
  }
  bool either = false;
  return prolong_rules(p, mask, rank, &either, rim);
}

bool stream_capturing(void* stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(reinterpret_cast<hipStream_t>(stream), &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  return cs != hipStreamCaptureStatusNone;
}

// The stream a solve runs on.  The legacy default stream cannot be captured: the solve then runs on an internal stream
// ordered after everything already queued on the default stream, and the destructor orders the default stream after it.
hipStream_t g_mg_stream = nullptr;
hipEvent_t g_mg_ev[2] = {nullptr, nullptr};
struct SolveStream {
  hipStream_t stream;
  const bool bridged;
  explicit SolveStream(hipStream_t user) : stream(user), bridged(!user) {
    if (!bridged) return;
    if (!g_mg_stream) {
      NEPTUNE_HIP_CHECK(hipStreamCreateWithFlags(&g_mg_stream, hipStreamNonBlocking));
      NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_mg_ev[0], hipEventDisableTiming));
      NEPTUNE_HIP_CHECK(hipEventCreateWithFlags(&g_mg_ev[1], hipEventDisableTiming));
    }
    NEPTUNE_HIP_CHECK(hipEventRecord(g_mg_ev[0], nullptr));
    NEPTUNE_HIP_CHECK(hipStreamWaitEvent(g_mg_stream, g_mg_ev[0], 0));
    stream = g_mg_stream;
  }
  ~SolveStream() {
    if (!bridged) return;
    NEPTUNE_HIP_CHECK(hipEventRecord(g_mg_ev[1], g_mg_stream));
    NEPTUNE_HIP_CHECK(hipStreamWaitEvent(nullptr, g_mg_ev[1], 0));
  }
  SolveStream(const SolveStream&) = delete;
  SolveStream& operator=(const SolveStream&) = delete;
};

int64_t g_mg_counts[3] = {0, 0, 0};   // plain cycles, graph cycles, checks of the last solve

// one solve, its arguments checked
struct Solve {
  const neptune_hip_mg_level_t* levels;
  const neptune_hip_mg_lines_t* lines;   // per level, or nullptr: no level has line stages
  int n_levels, dtype, rank, pre, post, coarse_sweeps;
  MgBox box[kMaxLevels];
  int mask[kMaxLevels];                  // mask[l]: how level l and l + 1 nest (sizes_nest: the axes, and the grid kind)
  bool linear[kMaxLevels];               // linear[l]: the pair (l, l + 1) prolongs linearly, by the rules rim[l]
  bool rlinear[kMaxLevels];              // rlinear[l]: it restricts by the transpose of that prolongation, same rules
  MgRim rim[kMaxLevels];
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
    cfg = (cfg_ && (cfg_->kernel || cfg_->variant >= 0 || cfg_->chunk || cfg_->flags)) ? cfg_ : nullptr;
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
        if ((L.body == NEPTUNE_HIP_BODY_LAP3D27_F32 ? NEPTUNE_HIP_F32 : NEPTUNE_HIP_F64) != dtype) return false;
      }
      if (L.g.num_inputs > 1 && !L.in_rest) return false;
      for (int i = 1; i < L.g.num_inputs; ++i)
        if (!L.in_rest[i - 1]) return false;
      if (l + 1 < n_levels && !isfinite(L.rscale)) return false;
      if (l > 0) {
        mask[l - 1] = sizes_nest(box[l - 1], box[l], rank);
        if (!mask[l - 1]) return false;
        linear[l - 1] = rlinear[l - 1] = false;
        if (transfer_ && !transfer_rules(transfer_[l - 1], mask[l - 1], rank, &linear[l - 1], &rlinear[l - 1], rim[l - 1])) return false;
        if (symmetric_only && linear[l - 1] != rlinear[l - 1]) return false;   // P must be a multiple of R^T
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
  // level l's inputs with `in0` as input 0
  void inputs(int l, const void* in0, const void** ins) const {
    const neptune_hip_mg_level_t& L = levels[l];
    ins[0] = in0;
    for (int i = 1; i < L.g.num_inputs; ++i) ins[i] = L.in_rest[i - 1];
  }
  // q_l = A_l(in0), a plain launch
  int apply_of(int l, const void* in0) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    inputs(l, in0, ins);
    const neptune_hip_launch_cfg_t* c = l == 0 ? cfg : nullptr;
    return L.fn ? L.fn(&L.g, ins, L.q, (void*)stream, c) : neptune_hip_apply_builtin(L.body, &L.g, ins, L.q, (void*)stream, c);
  }
  // q_l = A_l(x_l)
  int apply(int l) const { return apply_of(l, levels[l].x); }
  int stages(int l) const { return lines ? lines[l].n_stages : 0; }
  // stage `st` of level l: q = A(x), then the line kernel
  int line_stage(int l, int st) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const neptune_hip_mg_lines_t& S = lines[l];
    const int rc = apply(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    return do_line(dtype, box[l], S.axis[st] + 3 - rank, L.q, L.b, S.lo[st], S.inv[st], S.up[st], L.x, stream);
  }
  // `count` sweeps: the point sweep with minv, or on a level with k >= 1 line stages all k, each after its own apply --
  // stages 0 .. k-1, or k-1 .. 0 when `reversed` (the post-sweeps: a cycle of symmetric stages stays symmetric)
  int sweeps(int l, int count, bool reversed = false) const {
    const neptune_hip_mg_level_t& L = levels[l];
    const int k = lines ? lines[l].n_stages : 0;
    for (int s = 0; s < count; ++s) {
      for (int t = 0; t < std::max(k, 1); ++t) {
        int rc = apply(l);
        if (rc != NEPTUNE_HIP_OK) return rc;
        if (k == 0) {
          rc = do_smooth(dtype, box[l], L.q, L.b, L.minv, L.x, stream);
        } else {
          const neptune_hip_mg_lines_t& S = lines[l];
          const int st = reversed ? k - 1 - t : t;
          rc = do_line(dtype, box[l], S.axis[st] + 3 - rank, L.q, L.b, S.lo[st], S.inv[st], S.up[st], L.x, stream);
        }
        if (rc != NEPTUNE_HIP_OK) return rc;
      }
    }
    return NEPTUNE_HIP_OK;
  }
  // the two transfers of the pair (l, l + 1), each by the pair's choice
  int restrict_pair(int l) const {
    const neptune_hip_mg_level_t& F = levels[l];
    const neptune_hip_mg_level_t& Cl = levels[l + 1];
    return rlinear[l] ? do_restrict_linear(dtype, mask[l], box[l], box[l + 1], rim[l], F.b, F.q, F.rscale, Cl.b, Cl.x, stream)
                      : do_restrict(dtype, mask[l], box[l], box[l + 1], F.b, F.q, F.rscale, Cl.b, Cl.x, stream);
  }
  int prolong_pair(int l) const {
    const neptune_hip_mg_level_t& F = levels[l];
    const neptune_hip_mg_level_t& Cl = levels[l + 1];
    return linear[l] ? do_prolong_linear(dtype, mask[l], box[l], box[l + 1], rim[l], Cl.x, F.x, stream)
                     : do_prolong(dtype, mask[l], box[l], box[l + 1], Cl.x, F.x, stream);
  }
  int cycle(int l) const {
    if (l == n_levels - 1) return sweeps(l, coarse_sweeps);
    int rc = sweeps(l, pre);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = apply(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = restrict_pair(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = cycle(l + 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = prolong_pair(l);
    if (rc != NEPTUNE_HIP_OK) return rc;
    return sweeps(l, post, true);
  }
  // rr = sum over Omega_0 of (b - A(x))^2 into *rr_dev, then read back: one stream synchronise, one scalar
  int residual(void* rr_dev, double* rr) const {
    int rc = apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = neptune_hip_update_norm(dtype, &levels[0].g, levels[0].b, levels[0].q, rr_dev, (void*)stream);
    if (rc != NEPTUNE_HIP_OK) return rc;
    double h64 = 0.0;
    float h32 = 0.0f;
    void* h = dtype == NEPTUNE_HIP_F64 ? (void*)&h64 : (void*)&h32;
    NEPTUNE_HIP_CHECK(hipMemcpyAsync(h, rr_dev, elem_size(dtype), hipMemcpyDeviceToHost, stream));
    NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
    *rr = dtype == NEPTUNE_HIP_F64 ? h64 : (double)h32;
    return NEPTUNE_HIP_OK;
  }
  // One cycle as a graph: captured on the stream (nothing runs), instantiated; nullptr when any launch refused under
  // capture or the runtime would not have the graph -- the caller goes on with plain launches.
  hipGraphExec_t capture(hipGraph_t* graph_out) const {
    *graph_out = nullptr;
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const int rc = cycle(0);
    hipGraph_t graph = nullptr;
    if (hipStreamEndCapture(stream, &graph) != hipSuccess) { (void)hipGetLastError(); graph = nullptr; }
    if (rc != NEPTUNE_HIP_OK || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      return nullptr;
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipGraphDestroy(graph);
      return nullptr;
    }
    *graph_out = graph;
    return exec;
  }
};

// a late refusal: after the first launch of a cycle the fields have moved
int late(int rc) { return rc == NEPTUNE_HIP_EUNSUPPORTED ? NEPTUNE_HIP_EINVAL : rc; }

bool graph_path_enabled() {
  const char* e = getenv("NEPTUNE_HIP_MG_GRAPH");
  return !(e && strcmp(e, "0") == 0);
}

// ---------------------------------------------------------------- multigrid-preconditioned conjugate gradients
// The device block of neptune_hip_mgcg_solve and neptune_hip_mg_smooth_dot: PcgScalars, then rz_0, then the partials of the
// solver's own kernels; grown on demand, never while a capture is under way.
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

int64_t grid_blocks(const dim3& g) { return (int64_t)g.x * g.y; }

bool region_is_whole(const neptune_hip_apply_geom_t* g) {
  bool whole = true;
  for (int d = 0; d < g->rank; ++d) whole = whole && g->region_lb[d] <= 0 && g->region_ub[d] >= g->out_ub[d] - g->out_lb[d];
  return whole;
}

// what neptune_hip_mgcg_solve is once its arguments are checked.  S: the solve over the hierarchy whose level 0 carries
// (z, r) for (x, b) -- the cycle of the preconditioner --, L0: the caller's level 0.
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
// The loop of an MGCG solve once its set-up has run, shared by the one-type and the mixed driver: blocks of check_every
// iterations, the first one as plain launches, then -- when at least two more may follow -- ONE capture of `iteration` as a
// linear graph that every later iteration replays; after each block read_rr(first, &rr) reads rr back (the block's one
// synchronise; `first`: rz_0 into g_mgcg_rz0 as well).  `fused` is the iteration's own flag (whether step 1 is the
// dot-monitored launch): what refused under capture may well run outside, so a failed capture restores it.
template <class Iteration, class ReadRr>
int mgcg_iterations(hipStream_t stream, const MgcgArgs& a, bool& fused, Iteration&& iteration, ReadRr&& read_rr) {
  double rr = 0.0;
  struct Graph {    // this call's graph of one iteration
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool fallback = false;
    ~Graph() {
      if (exec) (void)hipGraphExecDestroy(exec);
      if (graph) (void)hipGraphDestroy(graph);
    }
  } G;
  // One iteration as a graph: captured on the stream (nothing runs), instantiated; on any refusal under capture the graph is
  // discarded and the call goes on with plain launches
  auto capture = [&]() {
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return; }
    const bool was_fused = fused;
    const int rc = iteration();
    hipGraph_t graph = nullptr;
    if (hipStreamEndCapture(stream, &graph) != hipSuccess) { (void)hipGetLastError(); graph = nullptr; }
    if (rc != NEPTUNE_HIP_OK || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      fused = was_fused;   // what refused under capture may well run outside
      return;
    }
    if (hipGraphInstantiate(&G.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipGraphDestroy(graph);
      G.exec = nullptr;
      fused = was_fused;
      return;
    }
    G.graph = graph;
    G.fallback = !fused;
  };

  const bool graphs = graph_path_enabled();
  bool capture_tried = false, rz0_read = false;
  int64_t done = 0;
  while (done < a.max_iters) {
    const int64_t block = a.check_every < a.max_iters - done ? a.check_every : a.max_iters - done;
    for (int64_t c = 0; c < block; ++c, ++done) {
      if (done > 0 && graphs && !capture_tried && a.max_iters - done >= 2) {
        capture_tried = true;
        capture();
      }
      if (done > 0 && G.exec) {
        NEPTUNE_HIP_CHECK(hipGraphLaunch(G.exec, stream));
        ++g_mgcg_counts[1];
        if (G.fallback) ++g_mgcg_counts[2];
      } else {
        const int rc = iteration();
        if (rc != NEPTUNE_HIP_OK) return late(rc);
        ++g_mgcg_counts[0];
        if (!fused) ++g_mgcg_counts[2];
      }
      if (a.iters_done) *a.iters_done = done + 1;
    }
    read_rr(!rz0_read, &rr);
    rz0_read = true;
    ++g_mgcg_counts[3];
    if (a.rr_last) *a.rr_last = rr;
    if (rr <= a.tol2) break;   // false for a NaN: such a solve runs to max_iters
  }
  return NEPTUNE_HIP_OK;
}

template <class T>
int mgcg_solve_typed(const Solve& S, const neptune_hip_mg_level_t& L0, const MgcgArgs& a) {
  const hipStream_t stream = S.stream;
  const MgBox& B0 = S.box[0];
  const int64_t n = B0.n[0] * B0.n[1] * B0.n[2];
  T* const x = static_cast<T*>(L0.x);
  const T* const b = static_cast<const T*>(L0.b);
  T* const q = static_cast<T*>(L0.q);
  const T* const minv = static_cast<const T*>(L0.minv);
  T* const r = static_cast<T*>(a.work[0]);
  T* const p = static_cast<T*>(a.work[1]);
  T* const z = static_cast<T*>(a.work[2]);
  T* const tr = static_cast<T*>(a.trace);

  CgBoxParams P;
  for (int d = 0; d < 3; ++d) {
    P.n[d] = B0.n[d];
    P.lo[d] = B0.lo[d];
    P.hi[d] = B0.lo[d] + B0.m[d];
  }
  const int64_t init_chunk = (P.n[2] + 255) / 256;
  const dim3 init_grid = grid_for_blocks(P.n[0] * P.n[1] * init_chunk);
  // k0 >= 1: level 0 smooths with line stages: r is stored without z = minv r, the cycle starts with the
  // apply-free stage and ends with the stage that yields r . z
  const int k0 = S.stages(0);
  const neptune_hip_mg_lines_t* const ln0 = k0 ? &S.lines[0] : nullptr;
  const int dot_axis = k0 ? ln0->axis[0] + 3 - S.rank : 0;
  const FlatGrid upd = k0 ? flat_grid(n, sizeof(T), {p, q, x, r}) : flat_grid(n, sizeof(T), {p, q, minv, x, r, z}),
                 dir = flat_grid(n, sizeof(T), {z, p});
  const RowGrid sd = row_grid(B0);
  const int64_t dot_blocks = k0 ? grid_blocks(line_grid(B0, dot_axis).grid) : grid_blocks(sd.grid);
  const int64_t most = std::max<int64_t>({grid_blocks(init_grid), (int64_t)upd.blocks, dot_blocks});
  grow_mgcg_ws(kMgcgScalarBytes + (size_t)most * sizeof(T), (void*)stream);   // no capture is under way: the entry refused one
  PcgScalars<T>* const scal = static_cast<PcgScalars<T>*>(g_mgcg_ws);
  T* const rz0_dev = reinterpret_cast<T*>(static_cast<char*>(g_mgcg_ws) + kMgcgRz0Offset);
  T* const partials = reinterpret_cast<T*>(static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes);
  auto final_kernel = [&](int64_t count, int stage) {
    hipLaunchKernelGGL(neptune_mgcg_final<T>, dim3(1), dim3(256), 0, stream, (const T*)partials, count, scal, rz0_dev, tr, a.max_iters, stage);
  };
  // `count` device scalars from `dev` after everything queued on the stream: the one synchronise of a block
  auto read = [&](const T* dev, double* host, const T* dev2 = nullptr, double* host2 = nullptr) {
    T h = 0, h2 = 0;
    NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h, dev, sizeof(T), hipMemcpyDeviceToHost, stream));
    if (dev2) NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h2, dev2, sizeof(T), hipMemcpyDeviceToHost, stream));
    NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
    *host = (double)h;
    if (dev2) *host2 = (double)h2;
  };
  // the rest of M: everything of the cycle on A z = r after its first pre-sweep (z = minv r, stored with r); its last
  // post-sweep yields r . z, which `stage` of the bookkeeping kernel takes
  auto rest_of_cycle = [&](int stage) -> int {
    int rc = NEPTUNE_HIP_OK;
    if (k0) {   // the first pre-sweep: stage 0 without an apply, from z = 0; then its other stages
      rc = do_line_first(S.dtype, B0, dot_axis, r, ln0->lo[0], ln0->inv[0], ln0->up[0], z, stream);
      for (int st = 1; st < k0 && rc == NEPTUNE_HIP_OK; ++st) rc = S.line_stage(0, st);
      if (rc != NEPTUNE_HIP_OK) return rc;
    }
    rc = S.sweeps(0, a.sweeps - 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.restrict_pair(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.cycle(1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.prolong_pair(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.sweeps(0, a.sweeps - 1, true);
    for (int st = k0 - 1; st >= 1 && rc == NEPTUNE_HIP_OK; --st) rc = S.line_stage(0, st);   // the last post-sweep, down to stage 1
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    if (k0) {
      rc = do_line_dot(S.dtype, B0, dot_axis, q, r, ln0->lo[0], ln0->inv[0], ln0->up[0], z, partials, stream);
      if (rc != NEPTUNE_HIP_OK) return rc;
    } else {
      hipLaunchKernelGGL(neptune_mg_smooth_dot<T>, sd.grid, dim3(256), 0, stream, B0, sd.nchunk, (const T*)q, (const T*)r, minv, z, partials);
    }
    final_kernel(dot_blocks, stage);
    return launched();
  };

  // ---- set-up
  for (int l = 1; l < S.n_levels; ++l) NEPTUNE_HIP_CHECK(hipMemsetAsync(S.levels[l].x, 0, box_bytes(S.box[l], sizeof(T)), stream));
  if (!region_is_whole(&L0.g)) NEPTUNE_HIP_CHECK(hipMemsetAsync(q, 0, (size_t)n * sizeof(T), stream));
  // with line stages on level 0, z outside Omega_0 is the error equation's rim: zero-filled here, never written again
  if (k0) NEPTUNE_HIP_CHECK(hipMemsetAsync(z, 0, (size_t)n * sizeof(T), stream));
  int rc = S.apply_of(0, x);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (k0) hipLaunchKernelGGL((neptune_mgcg_init<T, false>), init_grid, dim3(256), 0, stream, P, init_chunk, b, (const T*)q, minv, r, z, partials);
  else hipLaunchKernelGGL(neptune_mgcg_init<T>, init_grid, dim3(256), 0, stream, P, init_chunk, b, (const T*)q, minv, r, z, partials);
  final_kernel(grid_blocks(init_grid), kMgcgStartRr);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  double rr = 0.0;
  read(&scal->rr, &rr);
  if (a.rr0) *a.rr0 = rr;
  if (a.rr_last) *a.rr_last = rr;
  if (rr <= a.tol2 || a.max_iters == 0) return NEPTUNE_HIP_OK;
  rc = rest_of_cycle(kMgcgStartRz);
  if (rc != NEPTUNE_HIP_OK) return late(rc);
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(p, z, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, stream));

  // ---- one iteration.  fused: q = A(p) and pq out of one dot-monitored launch; a refusal of that entry
  // (NEPTUNE_HIP_EUNSUPPORTED, nothing launched) is remembered: a plain launch and neptune_hip_dot from then on
  bool fused = L0.fn ? a.fn_dot != nullptr : true;
  auto iteration = [&]() -> int {
    int rc;
    if (fused) {
      const void* ins[NEPTUNE_HIP_MAX_INPUTS];
      S.inputs(0, p, ins);
      rc = L0.fn ? a.fn_dot(&L0.g, ins, q, &scal->pq, (void*)stream, S.cfg)
                 : neptune_hip_apply_builtin_dot(L0.body, &L0.g, ins, q, &scal->pq, (void*)stream, S.cfg);
      if (rc == NEPTUNE_HIP_EUNSUPPORTED) fused = false;
      else if (rc != NEPTUNE_HIP_OK) return rc;
    }
    if (!fused) {
      rc = S.apply_of(0, p);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      rc = neptune_hip_dot(S.dtype, &L0.g, q, p, &scal->pq, (void*)stream);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
    }
    if (k0) flat_launch(upd, stream, neptune_mgcg_update<T, true, false>, neptune_mgcg_update<T, false, false>, n, scal, p, q, minv, x, r, z, partials);
    else flat_launch(upd, stream, neptune_mgcg_update<T, true>, neptune_mgcg_update<T, false>, n, scal, p, q, minv, x, r, z, partials);
    final_kernel((int64_t)upd.blocks, kMgcgRr);
    rc = rest_of_cycle(kMgcgRz);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    flat_launch(dir, stream, neptune_mgcg_direction<T, true>, neptune_mgcg_direction<T, false>, n, scal, z, p);
    return launched();
  };

  return mgcg_iterations(stream, a, fused, iteration, [&](bool first, double* out) {
    if (first) read(&scal->rr, out, rz0_dev, &g_mgcg_rz0);
    else read(&scal->rr, out);
  });
}

// ---------------------------------------------------------------- mixed precision: CG in D around a cycle in S
// what neptune_hip_mgcg_solve_mixed is once its arguments are checked.  S: the solve over the inner hierarchy in S, whose
// level 0 carries (z32, r32) for (x, b); O: the outer operator in D with the caller's x, b and q; a.work = r, p in D; cfg: the
// outer operator's launch configuration (nullptr unless the caller set anything).  Level 0
// has no line stages (the entry refused them).
template <class D, class Sx>
int mgcg_solve_mixed_typed(const Solve& S, const neptune_hip_mg_level_t& O, const neptune_hip_launch_cfg_t* cfg, const MgcgArgs& a) {
  const hipStream_t stream = S.stream;
  const MgBox& B0 = S.box[0];
  const neptune_hip_mg_level_t& F = S.levels[0];
  const int64_t n = B0.n[0] * B0.n[1] * B0.n[2];
  D* const x = static_cast<D*>(O.x);
  const D* const b = static_cast<const D*>(O.b);
  D* const q = static_cast<D*>(O.q);
  D* const r = static_cast<D*>(a.work[0]);
  D* const p = static_cast<D*>(a.work[1]);
  D* const tr = static_cast<D*>(a.trace);
  const Sx* const minv = static_cast<const Sx*>(F.minv);
  Sx* const r32 = static_cast<Sx*>(F.b);
  Sx* const z32 = static_cast<Sx*>(F.x);

  CgBoxParams P;
  for (int d = 0; d < 3; ++d) {
    P.n[d] = B0.n[d];
    P.lo[d] = B0.lo[d];
    P.hi[d] = B0.lo[d] + B0.m[d];
  }
  const int64_t init_chunk = (P.n[2] + 255) / 256;
  const dim3 init_grid = grid_for_blocks(P.n[0] * P.n[1] * init_chunk);
  const FlatGrid upd = flat_grid_group(n, kMixedGroup, {p, q, minv, x, r, r32, z32}), dir = flat_grid_group(n, kMixedGroup, {z32, p});
  const RowGrid sd = row_grid(B0);
  const int64_t most = std::max<int64_t>({grid_blocks(init_grid), (int64_t)upd.blocks, grid_blocks(sd.grid)});
  grow_mgcg_ws(kMgcgScalarBytes + (size_t)most * sizeof(D), (void*)stream);   // no capture is under way: the entry refused one
  PcgScalars<D>* const scal = static_cast<PcgScalars<D>*>(g_mgcg_ws);
  D* const rz0_dev = reinterpret_cast<D*>(static_cast<char*>(g_mgcg_ws) + kMgcgRz0Offset);
  D* const partials = reinterpret_cast<D*>(static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes);
  auto final_kernel = [&](int64_t count, int stage) {
    hipLaunchKernelGGL(neptune_mgcg_final<D>, dim3(1), dim3(256), 0, stream, (const D*)partials, count, scal, rz0_dev, tr, a.max_iters, stage);
  };
  auto read = [&](const D* dev, double* host, const D* dev2 = nullptr, double* host2 = nullptr) {
    D h = 0, h2 = 0;
    NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h, dev, sizeof(D), hipMemcpyDeviceToHost, stream));
    if (dev2) NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h2, dev2, sizeof(D), hipMemcpyDeviceToHost, stream));
    NEPTUNE_HIP_CHECK(hipStreamSynchronize(stream));
    *host = (double)h;
    if (dev2) *host2 = (double)h2;
  };
  // q = A(in0) by the outer operator, a plain launch in D
  auto outer_inputs = [&](const void* in0, const void** ins) {
    ins[0] = in0;
    for (int i = 1; i < O.g.num_inputs; ++i) ins[i] = O.in_rest[i - 1];
  };
  auto outer_apply = [&](const void* in0) -> int {
    const void* ins[NEPTUNE_HIP_MAX_INPUTS];
    outer_inputs(in0, ins);
    return O.fn ? O.fn(&O.g, ins, q, (void*)stream, cfg) : neptune_hip_apply_builtin(O.body, &O.g, ins, q, (void*)stream, cfg);
  };
  // the rest of M32: the cycle in S on A z32 = r32 after its first pre-sweep (z32 = minv r32, stored with r32); its last
  // post-sweep yields r32 . z32 in D, which `stage` of the bookkeeping kernel takes
  auto rest_of_cycle = [&](int stage) -> int {
    int rc = S.sweeps(0, a.sweeps - 1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.restrict_pair(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.cycle(1);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.prolong_pair(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.sweeps(0, a.sweeps - 1, true);
    if (rc != NEPTUNE_HIP_OK) return rc;
    rc = S.apply(0);
    if (rc != NEPTUNE_HIP_OK) return rc;
    hipLaunchKernelGGL((neptune_mg_smooth_dot_wide<D, Sx>), sd.grid, dim3(256), 0, stream, B0, sd.nchunk, static_cast<const Sx*>(F.q),
                       (const Sx*)r32, minv, z32, partials);
    final_kernel(grid_blocks(sd.grid), stage);
    return launched();
  };

  // ---- set-up
  for (int l = 1; l < S.n_levels; ++l) NEPTUNE_HIP_CHECK(hipMemsetAsync(S.levels[l].x, 0, box_bytes(S.box[l], sizeof(Sx)), stream));
  if (!region_is_whole(&O.g)) NEPTUNE_HIP_CHECK(hipMemsetAsync(q, 0, (size_t)n * sizeof(D), stream));
  int rc = outer_apply(x);
  if (rc != NEPTUNE_HIP_OK) return rc;
  hipLaunchKernelGGL((neptune_mgcg_init_mixed<D, Sx>), init_grid, dim3(256), 0, stream, P, init_chunk, b, (const D*)q, minv, r, r32, z32, partials);
  final_kernel(grid_blocks(init_grid), kMgcgStartRr);
  NEPTUNE_HIP_CHECK(hipGetLastError());
  double rr = 0.0;
  read(&scal->rr, &rr);
  if (a.rr0) *a.rr0 = rr;
  if (a.rr_last) *a.rr_last = rr;
  if (rr <= a.tol2 || a.max_iters == 0) return NEPTUNE_HIP_OK;
  rc = rest_of_cycle(kMgcgStartRz);
  if (rc != NEPTUNE_HIP_OK) return late(rc);
  flat_launch(dir, stream, neptune_mgcg_direction_mixed<D, Sx, true, true>, neptune_mgcg_direction_mixed<D, Sx, false, true>, n, scal, z32, p);

  // ---- one iteration; `fused` as in mgcg_solve_typed, on the outer operator
  bool fused = O.fn ? a.fn_dot != nullptr : true;
  auto iteration = [&]() -> int {
    int rc;
    if (fused) {
      const void* ins[NEPTUNE_HIP_MAX_INPUTS];
      outer_inputs(p, ins);
      rc = O.fn ? a.fn_dot(&O.g, ins, q, &scal->pq, (void*)stream, cfg)
                : neptune_hip_apply_builtin_dot(O.body, &O.g, ins, q, &scal->pq, (void*)stream, cfg);
      if (rc == NEPTUNE_HIP_EUNSUPPORTED) fused = false;
      else if (rc != NEPTUNE_HIP_OK) return rc;
    }
    if (!fused) {
      rc = outer_apply(p);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
      rc = neptune_hip_dot(NEPTUNE_HIP_F64, &O.g, q, p, &scal->pq, (void*)stream);
      if (rc != NEPTUNE_HIP_OK) return late(rc);
    }
    flat_launch(upd, stream, neptune_mgcg_update_mixed<D, Sx, true>, neptune_mgcg_update_mixed<D, Sx, false>, n, scal, p, q, minv, x, r, r32, z32,
                partials);
    final_kernel((int64_t)upd.blocks, kMgcgRr);
    rc = rest_of_cycle(kMgcgRz);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    flat_launch(dir, stream, neptune_mgcg_direction_mixed<D, Sx, true>, neptune_mgcg_direction_mixed<D, Sx, false>, n, scal, z32, p);
    return launched();
  };

  return mgcg_iterations(stream, a, fused, iteration, [&](bool first, double* out) {
    if (first) read(&scal->rr, out, rz0_dev, &g_mgcg_rz0);
    else read(&scal->rr, out);
  });
}

}  // namespace

extern "C" {

int neptune_hip_mg_smooth(int dtype, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                          void* stream) {
  if (!g || !q || !b || !minv || !x || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, elem_size(dtype));
  if (buffers_overlap(x, bytes, q, bytes) || buffers_overlap(x, bytes, b, bytes) || buffers_overlap(x, bytes, minv, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_smooth(dtype, B, q, b, minv, x, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_line_smooth(int dtype, const neptune_hip_apply_geom_t* g, int axis, void* q, const void* b, const void* lo,
                               const void* inv, const void* up, void* x, void* stream) {
  if (!g || !q || !b || !lo || !inv || !up || !x || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B) || axis < 0 || axis >= g->rank) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, elem_size(dtype));
  for (const void* f : {(const void*)q, b, lo, inv, up})
    if (buffers_overlap(x, bytes, f, bytes)) return NEPTUNE_HIP_EINVAL;
  for (const void* f : {b, lo, inv, up})
    if (buffers_overlap(q, bytes, f, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_line(dtype, B, axis + 3 - g->rank, q, b, lo, inv, up, x, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_line_first(int dtype, const neptune_hip_apply_geom_t* g, int axis, const void* b, const void* lo, const void* inv,
                              const void* up, void* x, void* stream) {
  if (!g || !b || !lo || !inv || !up || !x || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B) || axis < 0 || axis >= g->rank) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, elem_size(dtype));
  for (const void* f : {b, lo, inv, up})
    if (buffers_overlap(x, bytes, f, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_line_first(dtype, B, axis + 3 - g->rank, b, lo, inv, up, x, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_line_smooth_dot(int dtype, const neptune_hip_apply_geom_t* g, int axis, void* q, const void* b, const void* lo,
                                   const void* inv, const void* up, void* x, void* dot_out, void* stream) {
  if (!g || !q || !b || !lo || !inv || !up || !x || !dot_out || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B) || axis < 0 || axis >= g->rank) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype), bytes = box_bytes(B, elem);
  for (const void* f : {(const void*)q, b, lo, inv, up})
    if (buffers_overlap(x, bytes, f, bytes)) return NEPTUNE_HIP_EINVAL;
  for (const void* f : {b, lo, inv, up})
    if (buffers_overlap(q, bytes, f, bytes)) return NEPTUNE_HIP_EINVAL;
  if ((uintptr_t)dot_out % elem != 0) return NEPTUNE_HIP_EINVAL;
  for (const void* f : {(const void*)q, b, lo, inv, up, (const void*)x})
    if (buffers_overlap(dot_out, elem, f, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const int box_axis = axis + 3 - g->rank;
  const int64_t blocks = grid_blocks(line_grid(B, box_axis).grid);
  if (!grow_mgcg_ws(kMgcgScalarBytes + (size_t)blocks * elem, stream)) return NEPTUNE_HIP_EUNSUPPORTED;
  void* const partials = static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = do_line_dot(dtype, B, box_axis, q, b, lo, inv, up, x, partials, s);
  if (rc != NEPTUNE_HIP_OK) return rc;
  return by_type(dtype,
                 [&] {
                   hipLaunchKernelGGL(neptune_monitor_final<double>, dim3(1), dim3(256), 0, s, static_cast<const double*>(partials), blocks,
                                      static_cast<double*>(dot_out));
                   return launched();
                 },
                 [&] {
                   hipLaunchKernelGGL(neptune_monitor_final<float>, dim3(1), dim3(256), 0, s, static_cast<const float*>(partials), blocks,
                                      static_cast<float*>(dot_out));
                   return launched();
                 });
}

int neptune_hip_mg_restrict(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                            const void* b_fine, const void* q_fine, double rscale, void* b_coarse, void* x_coarse, void* stream) {
  if (!g_fine || !g_coarse || !b_fine || !q_fine || !b_coarse || !x_coarse || !known_dtype(dtype) || !isfinite(rscale)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  const int mask = g_fine->rank == g_coarse->rank ? sizes_nest(F, Cb, g_fine->rank) : 0;
  if (!mask) return NEPTUNE_HIP_EINVAL;
  const size_t fb = box_bytes(F, elem_size(dtype)), cb = box_bytes(Cb, elem_size(dtype));
  if (buffers_overlap(b_coarse, cb, x_coarse, cb)) return NEPTUNE_HIP_EINVAL;
  for (const void* w : {(const void*)b_coarse, (const void*)x_coarse})
    if (buffers_overlap(w, cb, b_fine, fb) || buffers_overlap(w, cb, q_fine, fb)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_restrict(dtype, mask, F, Cb, b_fine, q_fine, rscale, b_coarse, x_coarse, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_prolong_add(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                               const void* x_coarse, void* x_fine, void* stream) {
  if (!g_fine || !g_coarse || !x_coarse || !x_fine || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  const int mask = g_fine->rank == g_coarse->rank ? sizes_nest(F, Cb, g_fine->rank) : 0;
  if (!mask) return NEPTUNE_HIP_EINVAL;
  if (buffers_overlap(x_fine, box_bytes(F, elem_size(dtype)), x_coarse, box_bytes(Cb, elem_size(dtype)))) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  return do_prolong(dtype, mask, F, Cb, x_coarse, x_fine, reinterpret_cast<hipStream_t>(stream));
}

int neptune_hip_mg_prolong_add_linear(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                                      const neptune_hip_mg_prolong_t* p, const void* x_coarse, void* x_fine, void* stream) {
  if (!g_fine || !g_coarse || !p || !x_coarse || !x_fine || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  const int mask = g_fine->rank == g_coarse->rank ? sizes_nest(F, Cb, g_fine->rank) : 0;
  if (!mask) return NEPTUNE_HIP_EINVAL;
  bool linear = false;
  MgRim rim;
  if (!prolong_rules(*p, mask, g_fine->rank, &linear, rim)) return NEPTUNE_HIP_EINVAL;
  if (buffers_overlap(x_fine, box_bytes(F, elem_size(dtype)), x_coarse, box_bytes(Cb, elem_size(dtype)))) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return linear ? do_prolong_linear(dtype, mask, F, Cb, rim, x_coarse, x_fine, s) : do_prolong(dtype, mask, F, Cb, x_coarse, x_fine, s);
}

int neptune_hip_mg_restrict_linear(int dtype, const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse,
                                   const neptune_hip_mg_transfer_t* t, const void* b_fine, const void* q_fine, double rscale, void* b_coarse,
                                   void* x_coarse, void* stream) {
  if (!g_fine || !g_coarse || !t || !b_fine || !q_fine || !b_coarse || !x_coarse || !known_dtype(dtype) || !isfinite(rscale)) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb)) return NEPTUNE_HIP_EINVAL;
  const int mask = g_fine->rank == g_coarse->rank ? sizes_nest(F, Cb, g_fine->rank) : 0;
  if (!mask) return NEPTUNE_HIP_EINVAL;
  bool linear = false, rlinear = false;
  MgRim rim;
  if (!transfer_rules(*t, mask, g_fine->rank, &linear, &rlinear, rim)) return NEPTUNE_HIP_EINVAL;
  const size_t fb = box_bytes(F, elem_size(dtype)), cb = box_bytes(Cb, elem_size(dtype));
  if (buffers_overlap(b_coarse, cb, x_coarse, cb)) return NEPTUNE_HIP_EINVAL;
  for (const void* w : {(const void*)b_coarse, (const void*)x_coarse})
    if (buffers_overlap(w, cb, b_fine, fb) || buffers_overlap(w, cb, q_fine, fb)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return rlinear ? do_restrict_linear(dtype, mask, F, Cb, rim, b_fine, q_fine, rscale, b_coarse, x_coarse, s)
                 : do_restrict(dtype, mask, F, Cb, b_fine, q_fine, rscale, b_coarse, x_coarse, s);
}

int neptune_hip_mg_coarsened_axes(const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse, int* mask_out) {
  if (!g_fine || !g_coarse || !mask_out) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb) || g_fine->rank != g_coarse->rank) return NEPTUNE_HIP_EINVAL;
  const int mask = sizes_nest(F, Cb, g_fine->rank);
  if (!mask) return NEPTUNE_HIP_EINVAL;
  *mask_out = (mask & 7) >> (3 - g_fine->rank);   // the kernels' axes are the dimensions right-aligned
  return NEPTUNE_HIP_OK;
}

int neptune_hip_mg_halved_axes(const neptune_hip_apply_geom_t* g_fine, const neptune_hip_apply_geom_t* g_coarse, int* mask_out) {
  if (!g_fine || !g_coarse || !mask_out) return NEPTUNE_HIP_EINVAL;
  MgBox F, Cb;
  if (!level_box(g_fine, F) || !level_box(g_coarse, Cb) || g_fine->rank != g_coarse->rank) return NEPTUNE_HIP_EINVAL;
  const int mask = sizes_nest(F, Cb, g_fine->rank);
  if (!mask) return NEPTUNE_HIP_EINVAL;
  *mask_out = (mask & kMgCell) ? (mask & 7) >> (3 - g_fine->rank) : 0;
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
  for (int l = 0; have && l + 1 < n_levels; ++l) {
    tr[l].prolong = prolong[l].kind;
    tr[l].restrict_kind = NEPTUNE_HIP_MG_RESTRICT_AVERAGE;
    for (int d = 0; d < 3; ++d) {
      tr[l].rim_lo[d] = prolong[l].rim_lo[d];
      tr[l].rim_hi[d] = prolong[l].rim_hi[d];
    }
  }
  return neptune_hip_mg_solve_transfer(levels, lines, have ? tr : nullptr, n_levels, dtype, pre, post, coarse_sweeps, max_cycles, check_every,
                                       tol2, rr_checks, stream, cfg, cycles_done, rr0, rr_last);
}

int neptune_hip_mg_solve_transfer(const neptune_hip_mg_level_t* levels, const neptune_hip_mg_lines_t* lines,
                                  const neptune_hip_mg_transfer_t* transfer, int n_levels, int dtype, int pre, int post, int coarse_sweeps,
                                  int64_t max_cycles, int64_t check_every, double tol2, double* rr_checks, void* stream,
                                  const neptune_hip_launch_cfg_t* cfg, int64_t* cycles_done, double* rr0, double* rr_last) {
  g_mg_counts[0] = g_mg_counts[1] = g_mg_counts[2] = 0;
  if (cycles_done) *cycles_done = 0;
  if (rr0) *rr0 = 0.0;
  if (rr_last) *rr_last = 0.0;
  // ---- the refusals, before anything touches the device
  if (check_every < 1 || max_cycles < 0) return NEPTUNE_HIP_EINVAL;
  Solve S;
  if (!S.check(levels, n_levels, dtype, pre, post, coarse_sweeps, cfg, lines, transfer)) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype);
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  SolveStream sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  struct Scalar {   // one device T for r . r, this call's
    void* p = nullptr;
    Scalar() { NEPTUNE_HIP_CHECK(hipMalloc(&p, 8)); }
    ~Scalar() { (void)hipFree(p); }
  } rr_dev;
  struct Graph {    // this call's graph of one cycle
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~Graph() {
      if (exec) (void)hipGraphExecDestroy(exec);
      if (graph) (void)hipGraphDestroy(graph);
    }
  } G;

  for (int l = 1; l < n_levels; ++l) NEPTUNE_HIP_CHECK(hipMemsetAsync(levels[l].x, 0, box_bytes(S.box[l], elem), S.stream));
  double rr = 0.0;
  int rc = S.residual(rr_dev.p, &rr);
  if (rc != NEPTUNE_HIP_OK) return rc;
  if (rr0) *rr0 = rr;
  if (rr_last) *rr_last = rr;
  if (rr <= tol2) return NEPTUNE_HIP_OK;

  const bool graphs = graph_path_enabled();
  bool capture_tried = false;
  int64_t done = 0;
  while (done < max_cycles) {
    const int64_t block = check_every < max_cycles - done ? check_every : max_cycles - done;
    for (int64_t c = 0; c < block; ++c, ++done) {
      // the first cycle plain: it validates the request and lets first-use tuning run outside capture; then, when at least
      // two more cycles may follow, ONE capture
      if (done > 0 && graphs && !capture_tried && max_cycles - done >= 2) {
        capture_tried = true;
        G.exec = S.capture(&G.graph);
      }
      if (done > 0 && G.exec) {
        NEPTUNE_HIP_CHECK(hipGraphLaunch(G.exec, S.stream));
        ++g_mg_counts[1];
      } else {
        rc = S.cycle(0);
        if (rc != NEPTUNE_HIP_OK) return late(rc);
        ++g_mg_counts[0];
      }
      if (cycles_done) *cycles_done = done + 1;
    }
    rc = S.residual(rr_dev.p, &rr);
    if (rc != NEPTUNE_HIP_OK) return late(rc);
    if (rr_checks) rr_checks[g_mg_counts[2]] = rr;
    ++g_mg_counts[2];
    if (rr_last) *rr_last = rr;
    if (rr <= tol2) break;   // false for a NaN: such a solve runs to max_cycles
  }
  return NEPTUNE_HIP_OK;
}

int neptune_hip_mg_smooth_dot(int dtype, const neptune_hip_apply_geom_t* g, const void* q, const void* b, const void* minv, void* x,
                              void* dot_out, void* stream) {
  if (!g || !q || !b || !minv || !x || !dot_out || !known_dtype(dtype)) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype), bytes = box_bytes(B, elem);
  if (buffers_overlap(x, bytes, q, bytes) || buffers_overlap(x, bytes, b, bytes) || buffers_overlap(x, bytes, minv, bytes)) return NEPTUNE_HIP_EINVAL;
  if ((uintptr_t)dot_out % elem != 0) return NEPTUNE_HIP_EINVAL;
  for (const void* f : {q, b, minv, (const void*)x})
    if (buffers_overlap(dot_out, elem, f, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const RowGrid r = row_grid(B);
  const int64_t blocks = grid_blocks(r.grid);
  if (!grow_mgcg_ws(kMgcgScalarBytes + (size_t)blocks * elem, stream)) return NEPTUNE_HIP_EUNSUPPORTED;
  void* const partials = static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return by_type(dtype,
                 [&] {
                   hipLaunchKernelGGL(neptune_mg_smooth_dot<double>, r.grid, dim3(256), 0, s, B, r.nchunk, static_cast<const double*>(q),
                                      static_cast<const double*>(b), static_cast<const double*>(minv), static_cast<double*>(x),
                                      static_cast<double*>(partials));
                   hipLaunchKernelGGL(neptune_monitor_final<double>, dim3(1), dim3(256), 0, s, static_cast<const double*>(partials), blocks,
                                      static_cast<double*>(dot_out));
                   return launched();
                 },
                 [&] {
                   hipLaunchKernelGGL(neptune_mg_smooth_dot<float>, r.grid, dim3(256), 0, s, B, r.nchunk, static_cast<const float*>(q),
                                      static_cast<const float*>(b), static_cast<const float*>(minv), static_cast<float*>(x),
                                      static_cast<float*>(partials));
                   hipLaunchKernelGGL(neptune_monitor_final<float>, dim3(1), dim3(256), 0, s, static_cast<const float*>(partials), blocks,
                                      static_cast<float*>(dot_out));
                   return launched();
                 });
}

int neptune_hip_mg_smooth_dot_wide(int dtype, int dtype_sum, const neptune_hip_apply_geom_t* g, const void* q, const void* b,
                                   const void* minv, void* x, void* dot_out, void* stream) {
  if (!g || !q || !b || !minv || !x || !dot_out || dtype != NEPTUNE_HIP_F32 || dtype_sum != NEPTUNE_HIP_F64) return NEPTUNE_HIP_EINVAL;
  MgBox B;
  if (!level_box(g, B)) return NEPTUNE_HIP_EINVAL;
  const size_t bytes = box_bytes(B, sizeof(float));
  if (buffers_overlap(x, bytes, q, bytes) || buffers_overlap(x, bytes, b, bytes) || buffers_overlap(x, bytes, minv, bytes)) return NEPTUNE_HIP_EINVAL;
  if ((uintptr_t)dot_out % sizeof(double) != 0) return NEPTUNE_HIP_EINVAL;
  for (const void* f : {q, b, minv, (const void*)x})
    if (buffers_overlap(dot_out, sizeof(double), f, bytes)) return NEPTUNE_HIP_EINVAL;
  ensure_init();
  const RowGrid r = row_grid(B);
  const int64_t blocks = grid_blocks(r.grid);
  if (!grow_mgcg_ws(kMgcgScalarBytes + (size_t)blocks * sizeof(double), stream)) return NEPTUNE_HIP_EUNSUPPORTED;
  double* const partials = reinterpret_cast<double*>(static_cast<char*>(g_mgcg_ws) + kMgcgScalarBytes);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((neptune_mg_smooth_dot_wide<double, float>), r.grid, dim3(256), 0, s, B, r.nchunk, static_cast<const float*>(q),
                     static_cast<const float*>(b), static_cast<const float*>(minv), static_cast<float*>(x), partials);
  hipLaunchKernelGGL(neptune_monitor_final<double>, dim3(1), dim3(256), 0, s, (const double*)partials, blocks, static_cast<double*>(dot_out));
  return launched();
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
  g_mgcg_counts[0] = g_mgcg_counts[1] = g_mgcg_counts[2] = g_mgcg_counts[3] = 0;
  g_mgcg_rz0 = 0.0;
  if (iters_done) *iters_done = 0;
  if (rr0) *rr0 = 0.0;
  if (rr_last) *rr_last = 0.0;
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
  // the fields of both precisions that the solve touches on levels 0 and 1, the trace included: none may meet another (each
  // inner level's own four were checked against each other and the neighbour's above)
  struct Span { const void* p; size_t bytes; size_t align; };
  const size_t wide0 = box_bytes(OB, sizeof(double)), narrow0 = box_bytes(S.box[0], sizeof(float)), narrow1 = box_bytes(S.box[1], sizeof(float));
  const Span spans[14] = {{O.x, wide0, 8},           {O.b, wide0, 8},           {O.q, wide0, 8},           {work[0], wide0, 8},
                          {work[1], wide0, 8},       {trace, (size_t)(3 * max_iters) * sizeof(double), 8},
                          {levels[0].x, narrow0, 4}, {levels[0].b, narrow0, 4}, {levels[0].q, narrow0, 4}, {levels[0].minv, narrow0, 4},
                          {levels[1].x, narrow1, 4}, {levels[1].b, narrow1, 4}, {levels[1].q, narrow1, 4}, {levels[1].minv, narrow1, 4}};
  for (int i = 0; i < 14; ++i) {
    const bool optional = i == 5 || i == 9 || i == 13;   // the trace; minv of a level with line stages
    if (!spans[i].p) {
      if (optional) continue;
      return NEPTUNE_HIP_EINVAL;
    }
    if ((uintptr_t)spans[i].p % spans[i].align != 0) return NEPTUNE_HIP_EINVAL;
    for (int o = 0; o < (i < 6 ? i : 6); ++o)   // an inner field against the wide ones and the trace only
      if (spans[o].p && buffers_overlap(spans[i].p, spans[i].bytes, spans[o].p, spans[o].bytes)) return NEPTUNE_HIP_EINVAL;
  }
  // line stages on level 0 need a wide-sum form of both code paths of the line kernel: not built yet
  if (S.stages(0) > 0) return NEPTUNE_HIP_EUNSUPPORTED;
  // the factor fields are read while x, q, r, p and the trace are written: they may meet none of them
  for (int l = 0; l < n_levels && lines; ++l)
    for (int st = 0; st < lines[l].n_stages; ++st)
      for (const void* f : {lines[l].lo[st], lines[l].inv[st], lines[l].up[st]}) {
        const size_t fb = box_bytes(S.box[l], sizeof(float));
        for (int o = 0; o < 6; ++o)
          if (spans[o].p && buffers_overlap(f, fb, spans[o].p, spans[o].bytes)) return NEPTUNE_HIP_EINVAL;
      }
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  SolveStream sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  const neptune_hip_launch_cfg_t* const outer_cfg = (cfg && (cfg->kernel || cfg->variant >= 0 || cfg->chunk || cfg->flags)) ? cfg : nullptr;
  const MgcgArgs a = {fn_dot, sweeps, work, max_iters, check_every, tol2, trace, iters_done, rr0, rr_last};
  return mgcg_solve_mixed_typed<double, float>(S, O, outer_cfg, a);
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
  g_mgcg_counts[0] = g_mgcg_counts[1] = g_mgcg_counts[2] = g_mgcg_counts[3] = 0;
  g_mgcg_rz0 = 0.0;
  if (iters_done) *iters_done = 0;
  if (rr0) *rr0 = 0.0;
  if (rr_last) *rr_last = 0.0;
  // ---- the refusals, before anything touches the device
  if (n_levels < 2 || sweeps < 1 || check_every < 1 || max_iters < 0 || !work) return NEPTUNE_HIP_EINVAL;
  Solve S;
  if (!S.check(levels, n_levels, dtype, sweeps, sweeps, coarse_sweeps, cfg, lines, transfer, true)) return NEPTUNE_HIP_EINVAL;
  const size_t elem = elem_size(dtype);
  const size_t bytes0 = box_bytes(S.box[0], elem), bytes1 = box_bytes(S.box[1], elem), trace_bytes = (size_t)(3 * max_iters) * elem;
  const void* const fine[4] = {levels[0].x, levels[0].b, levels[0].q, levels[0].minv};
  const void* const coarse[4] = {levels[1].x, levels[1].b, levels[1].q, levels[1].minv};
  if (trace && (uintptr_t)trace % elem != 0) return NEPTUNE_HIP_EINVAL;
  for (int i = 0; i < 3; ++i) {
    if (!work[i] || (uintptr_t)work[i] % elem != 0) return NEPTUNE_HIP_EINVAL;
    for (int o = 0; o < i; ++o)
      if (buffers_overlap(work[i], bytes0, work[o], bytes0)) return NEPTUNE_HIP_EINVAL;
    for (int o = 0; o < 4; ++o)   // minv of a level with stages may be null
      if ((fine[o] && buffers_overlap(work[i], bytes0, fine[o], bytes0)) || (coarse[o] && buffers_overlap(work[i], bytes0, coarse[o], bytes1)))
        return NEPTUNE_HIP_EINVAL;
    if (trace && buffers_overlap(trace, trace_bytes, work[i], bytes0)) return NEPTUNE_HIP_EINVAL;
  }
  for (int o = 0; o < 4 && trace; ++o)
    if ((fine[o] && buffers_overlap(trace, trace_bytes, fine[o], bytes0)) || (coarse[o] && buffers_overlap(trace, trace_bytes, coarse[o], bytes1)))
      return NEPTUNE_HIP_EINVAL;
  // the factor fields are read while r, p, z and the trace are written: they may meet none of them
  for (int l = 0; l < n_levels && lines; ++l)
    for (int st = 0; st < lines[l].n_stages; ++st)
      for (const void* f : {lines[l].lo[st], lines[l].inv[st], lines[l].up[st]}) {
        const size_t fb = box_bytes(S.box[l], elem);
        for (int i = 0; i < 3; ++i)
          if (buffers_overlap(f, fb, work[i], bytes0)) return NEPTUNE_HIP_EINVAL;
        if (trace && buffers_overlap(f, fb, trace, trace_bytes)) return NEPTUNE_HIP_EINVAL;
      }
  // rr is read back after every block: not while the caller's stream is being captured
  if (stream_capturing(stream)) return NEPTUNE_HIP_EINVAL;

  ensure_init();
  SolveStream sc(reinterpret_cast<hipStream_t>(stream));
  S.stream = sc.stream;
  // the preconditioner's hierarchy: level 0 carries (z, r) for (x, b)
  neptune_hip_mg_level_t lv[kMaxLevels];
  for (int l = 0; l < n_levels; ++l) lv[l] = levels[l];
  lv[0].x = work[2];
  lv[0].b = work[0];
  S.levels = lv;
  const MgcgArgs a = {fn_dot, sweeps, work, max_iters, check_every, tol2, trace, iters_done, rr0, rr_last};
  return dtype == NEPTUNE_HIP_F64 ? mgcg_solve_typed<double>(S, levels[0], a) : mgcg_solve_typed<float>(S, levels[0], a);
}

}  // extern "C"
