// multigrid_kernels.hpp -- the kernels of the geometric multigrid V-cycle (neptune_hip_mg_solve):
//
//   neptune_mg_smooth        x = x + (minv * (b - q)) on Omega                       reads q, b, minv, x; writes x: 5 passes
//   neptune_mg_restrict      b_c = rscale * R(b_f - q_f), x_c = +0 on the coarse Omega   reads b_f, q_f once; writes 2 / 2^k (k axes coarsened)
//   neptune_mg_restrict_kept2   the same with the contiguous axis kept
//   neptune_mg_prolong_add   x_f = x_f + P(x_c) on the fine Omega                     reads and writes x_f; reads x_c through L1
//   neptune_mg_restrict_cell / neptune_mg_prolong_add_cell   the two transfers of a cell-centred pair (at the end)
//   neptune_mg_prolong_add_linear   the linear prolongation of a cell-centred pair, weights 3/4 and 1/4, a rule per face
//   neptune_mg_restrict_linear      its transpose / 2^k as the restriction, by the same rules
//
// Grids: vertex-centred, Dirichlet rim.  Per pair of levels every dimension is either COARSENED, m_fine = 2 m_coarse + 1: the
// coarse cell of interior index j sits on the fine cell of interior index 2 j + 1 (interior indices count from Omega's lower
// corner); or KEPT, m_fine = m_coarse: coarse j sits on fine j and the transfer along it is the identity (semi-coarsening,
// DESIGN 3.16).  The transfer kernels take the pair's state as a compile-time mask MASK: bit a (value 1 << a) set = axis a
// is coarsened; at least one bit is set.
//
// The frame, stated once.  Addressing is the rows form of krylov_kernels.hpp's box_cell, over Omega instead of the box: a
// workgroup owns ONE 256-cell chunk of one row of (the fine or the coarse) Omega, so the row decode is workgroup-uniform
// scalar work and only Omega's cells are ever addressed -- nothing outside is read or written.  Axes: every level's box is
// held on three axes with the field's dimensions RIGHT-aligned (rank 2: axes 1, 2; rank 1: axis 2), absent axes have extent
// 1 and are kept: full coarsening of rank 3, 2, 1 is MASK 7, 6, 4.  Axis 2 is the contiguous one.
// Arithmetic: everything in T, every intermediate a named temporary, one rounding per operation (build with
// -ffp-contract=off).  The transfer stencils run along axis 2 first, then axis 1, then axis 0, skipping kept axes.  No
// atomics, no reductions.
// Templates only: the translation unit that holds the solver instantiates them.
#pragma once
#include "apply_common.hpp"
#include "apply_march.hpp"   // the wave shifts from_prev / from_next

namespace neptune_hip {

// one level's box and Omega on the three axes
struct MgBox {
  int64_t n[3];    // the box's extents
  int64_t lo[3];   // Omega's lower corner, physical
  int64_t m[3];    // Omega's extents (>= 1)
};

// The row decode all three kernels share: workgroup `blk` owns chunk c of row (i, j) of B's Omega; -> false past the last
// workgroup of a folded grid (workgroup-uniform).  k = the lane's interior index along axis 2 (may be >= m[2]: no cell).
__device__ __forceinline__ bool mg_row(const MgBox& B, int64_t nchunk, int64_t blk, int64_t& i, int64_t& j, int64_t& k0) {
  if (blk >= B.m[0] * B.m[1] * nchunk) return false;
  const int64_t row = blk / nchunk, c = blk - row * nchunk;
  i = row / B.m[1];
  j = row - i * B.m[1];
  k0 = c * 256;
  return true;
}
// flat index of the cell with interior indices (i, j, k)
__device__ __forceinline__ int64_t mg_at(const MgBox& B, int64_t i, int64_t j, int64_t k) {
  return ((B.lo[0] + i) * B.n[1] + (B.lo[1] + j)) * B.n[2] + (B.lo[2] + k);
}

// ---------------------------------------------------------------- smoothing sweep
// On Omega: d = b - q, w = minv * d, x = x + w.  q = A(x) comes from the plain launch just before.
template <class T>
__global__ __launch_bounds__(256) void neptune_mg_smooth(MgBox B, int64_t nchunk, const T* __restrict__ q, const T* __restrict__ b,
                                                         const T* __restrict__ minv, T* __restrict__ x) {
  int64_t i, j, k0;
  if (!mg_row(B, nchunk, linear_block(), i, j, k0)) return;
  const int64_t k = k0 + threadIdx.x;
  if (k >= B.m[2]) return;
  const int64_t o = mg_at(B, i, j, k);
  const T d = b[o] - q[o];
  const T w = minv[o] * d;
  x[o] = x[o] + w;
}

// ---------------------------------------------------------------- restriction, fused with the residual
// the one-dimensional full-weighting stencil: two exact products, two rounded additions
template <class T>
__device__ __forceinline__ T mg_weigh(T am, T a0, T ap) {
  const T qm = (T)0.25 * am;
  const T h0 = (T)0.5 * a0;
  const T qp = (T)0.25 * ap;
  const T s = qm + h0;
  return s + qp;
}

// The workgroup owns coarse cells (ci, cj, ck0 .. ck0 + 255).  It needs d = b - q on the fine rows (2 ci + {0, 1, 2},
// 2 cj + {0, 1, 2}) at fine interior indices 2 ck0 .. 2 ck0 + 512 along axis 2: each such row segment is loaded ONCE by the
// workgroup, coalesced, differenced and staged in LDS (the rows of one fine plane side by side), from where every lane takes
// its three operands.  Rows and planes that neighbouring workgroups share (even fine indices) come out of L2.  Per fine plane
// the stencil runs along axis 2, then axis 1, in registers; the three planes are combined last.
constexpr int kMgRestrictRow = 2 * 256 + 1;   // fine cells of one staged row segment
constexpr int kMgRestrictPitch = kMgRestrictRow + 3;
// This kernel: axis 2 coarsened (MASK & 4); the row count NJ and the plane count NI follow bits 1 and 0.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_restrict(MgBox F, MgBox Cb, int64_t nchunk, const T* __restrict__ b_f,
                                                           const T* __restrict__ q_f, T rscale, T* __restrict__ b_c,
                                                           T* __restrict__ x_c) {
  static_assert((MASK & 4) != 0 && MASK < 8, "axis 2 coarsened");
  constexpr int NI = (MASK & 1) ? 3 : 1, NJ = (MASK & 2) ? 3 : 1;
  __shared__ T lds[NJ * kMgRestrictPitch];
  int64_t ci, cj, ck0;
  if (!mg_row(Cb, nchunk, linear_block(), ci, cj, ck0)) return;
  const int64_t ck = ck0 + threadIdx.x;
  const bool owns = ck < Cb.m[2];
  // the staged segment: fine interior indices [fk0, fk0 + len) along axis 2; the size relation keeps it inside Omega
  const int64_t fk0 = 2 * ck0;
  const int64_t rest = F.m[2] - fk0;
  const int len = (int)(rest < (int64_t)kMgRestrictRow ? rest : (int64_t)kMgRestrictRow);
  const int64_t fi0 = (MASK & 1) ? 2 * ci : ci, fj0 = (MASK & 2) ? 2 * cj : cj;
  T plane[NI];
#pragma unroll
  for (int a = 0; a < NI; ++a) {
    if (a > 0) __syncthreads();   // the previous plane's operands are in registers before its rows are overwritten
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
      const int64_t o = mg_at(F, fi0 + a, fj0 + r, fk0);
      for (int t = threadIdx.x; t < len; t += 256) {
        const T d = b_f[o + t] - q_f[o + t];
        lds[r * kMgRestrictPitch + t] = d;
      }
    }
    __syncthreads();
    T row[NJ];
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
      row[r] = (T)0;
      if (owns) {
        const T* s = lds + r * kMgRestrictPitch + 2 * (int)threadIdx.x;
        row[r] = mg_weigh(s[0], s[1], s[2]);
      }
    }
    if constexpr (NJ == 3) plane[a] = mg_weigh(row[0], row[1], row[2]);
    else plane[a] = row[0];
  }
  if (!owns) return;
  T t;
  if constexpr (NI == 3) t = mg_weigh(plane[0], plane[1], plane[2]);
  else t = plane[0];
  const int64_t oc = mg_at(Cb, ci, cj, ck);
  b_c[oc] = rscale * t;
  x_c[oc] = (T)0;
}

// Axis 2 kept (MASK = 1, 2, 3): the workgroup's 256 coarse cells sit on the same 256 interior indices of the fine rows
// (2 ci + {0, 1, 2} or ci, 2 cj + {0, 1, 2} or cj).  Every lane loads its own cell of the NI x NJ rows directly -- coalesced,
// nothing staged, no barrier -- and d = b - q goes through to the stencil along axis 1, then axis 0, unchanged.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_restrict_kept2(MgBox F, MgBox Cb, int64_t nchunk, const T* __restrict__ b_f,
                                                                 const T* __restrict__ q_f, T rscale, T* __restrict__ b_c,
                                                                 T* __restrict__ x_c) {
  static_assert((MASK & 4) == 0 && MASK > 0, "axis 2 kept, another one coarsened");
  constexpr int NI = (MASK & 1) ? 3 : 1, NJ = (MASK & 2) ? 3 : 1;
  int64_t ci, cj, ck0;
  if (!mg_row(Cb, nchunk, linear_block(), ci, cj, ck0)) return;
  const int64_t ck = ck0 + threadIdx.x;
  if (ck >= Cb.m[2]) return;
  const int64_t fi0 = (MASK & 1) ? 2 * ci : ci, fj0 = (MASK & 2) ? 2 * cj : cj;
  T plane[NI];
#pragma unroll
  for (int a = 0; a < NI; ++a) {
    T row[NJ];
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
      const int64_t o = mg_at(F, fi0 + a, fj0 + r, ck);
      row[r] = b_f[o] - q_f[o];
    }
    if constexpr (NJ == 3) plane[a] = mg_weigh(row[0], row[1], row[2]);
    else plane[a] = row[0];
  }
  T t;
  if constexpr (NI == 3) t = mg_weigh(plane[0], plane[1], plane[2]);
  else t = plane[0];
  const int64_t oc = mg_at(Cb, ci, cj, ck);
  b_c[oc] = rscale * t;
  x_c[oc] = (T)0;
}

// ---------------------------------------------------------------- prolongation and correction
// one-dimensional interpolation at a fine cell: odd interior index -> the coarse value `hi` itself; even -> 0.5 * (lo + hi),
// one rounded addition and the exact scaling.  (lo, hi) = e[i / 2 - 1], e[i / 2] for even i, and hi = e[(i - 1) / 2] for odd i;
// an operand on the rim is +0.
template <class T>
__device__ __forceinline__ T mg_interp(bool odd, T lo, T hi) {
  const T s = lo + hi;
  const T h = (T)0.5 * s;
  return odd ? hi : h;
}

// The workgroup owns fine cells (fi, fj, fk0 .. fk0 + 255).  Along axes 0 and 1 the parity is workgroup-uniform: on a
// coarsened axis an odd index needs one coarse row / plane, an even one two, of which one may be the rim; on a kept axis the
// one row / plane of the same index is read and there is no rim.  The coarse operands -- up to 2^(coarsened axes) per cell,
// consecutive lanes on consecutive or equal coarse cells of the same few rows -- are read through L1: the coarse field is
// that fraction of the fine one.  Axis 2 kept: consecutive lanes read consecutive coarse cells, one operand, no parity.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_prolong_add(MgBox F, MgBox Cb, int64_t nchunk, const T* __restrict__ x_c,
                                                              T* __restrict__ x_f) {
  static_assert(MASK > 0 && MASK < 8, "at least one axis coarsened");
  constexpr bool C0 = (MASK & 1) != 0, C1 = (MASK & 2) != 0, C2 = (MASK & 4) != 0;
  constexpr int NI = C0 ? 2 : 1, NJ = C1 ? 2 : 1;
  int64_t fi, fj, fk0;
  if (!mg_row(F, nchunk, linear_block(), fi, fj, fk0)) return;
  const int64_t fk = fk0 + threadIdx.x;
  if (fk >= F.m[2]) return;
  // per axis: the two coarse interior indices (lo, hi) and the parity; a kept axis takes its only index as `hi`
  const bool oi = C0 ? (fi & 1) != 0 : true, oj = C1 ? (fj & 1) != 0 : true, ok = C2 ? (fk & 1) != 0 : true;
  const int64_t ci[2] = {C0 ? fi / 2 - 1 : -1, C0 ? (oi ? (fi - 1) / 2 : fi / 2) : fi};
  const int64_t cj[2] = {C1 ? fj / 2 - 1 : -1, C1 ? (oj ? (fj - 1) / 2 : fj / 2) : fj};
  const int64_t ck[2] = {C2 ? fk / 2 - 1 : -1, C2 ? (ok ? (fk - 1) / 2 : fk / 2) : fk};
  // slot 0 (`lo`) is used on an even index only; an index outside [0, m) is the rim
  const bool vi[2] = {!oi && ci[0] >= 0, C0 ? ci[1] < Cb.m[0] : true}, vj[2] = {!oj && cj[0] >= 0, C1 ? cj[1] < Cb.m[1] : true};
  const bool vk[2] = {!ok && ck[0] >= 0, C2 ? ck[1] < Cb.m[2] : true};
  T ei[2] = {(T)0, (T)0};
#pragma unroll
  for (int a = 2 - NI; a < 2; ++a) {
    T ej[2] = {(T)0, (T)0};
#pragma unroll
    for (int r = 2 - NJ; r < 2; ++r) {
      T klo = (T)0, khi = (T)0;
      if (vi[a] && vj[r]) {
        if constexpr (C2) {
          if (vk[0]) klo = x_c[mg_at(Cb, ci[a], cj[r], ck[0])];
        }
        if (vk[1]) khi = x_c[mg_at(Cb, ci[a], cj[r], ck[1])];
      }
      ej[r] = C2 ? mg_interp(ok, klo, khi) : khi;
    }
    ei[a] = C1 ? mg_interp(oj, ej[0], ej[1]) : ej[1];
  }
  const T e = C0 ? mg_interp(oi, ei[0], ei[1]) : ei[1];
  const int64_t o = mg_at(F, fi, fj, fk);
  x_f[o] = x_f[o] + e;
}

// ================================================================ cell-centred pairs
// A dimension may be in a third state, HALVED: m_fine = 2 m_coarse, the coarse cell of interior index j covers the fine cells
// of interior index 2 j and 2 j + 1.  One pair of levels is one grid kind: the two kernels below take MASK = the HALVED axes
// (the others are kept; at least one bit is set) and never see a COARSENED one.  There is no rim operand: the restriction
// reads the fine Omega only, the prolongation the coarse Omega only.  Neither needs LDS or a barrier.

// the mean of a pair: one rounded addition and the exact scaling
template <class T>
__device__ __forceinline__ T mg_mean(T a0, T a1) {
  const T s = a0 + a1;
  return (T)0.5 * s;
}
// the cells p[0], p[1].  `aligned` (workgroup-uniform): p is a multiple of 2 sizeof(T) -- one load of twice the width;
// else two loads.  The same bits either way.
template <class T>
__device__ __forceinline__ void mg_load_pair(const T* p, bool aligned, T& a0, T& a1) {
  if (aligned) {
    T v[2];
    __builtin_memcpy(v, __builtin_assume_aligned(p, 2 * sizeof(T)), 2 * sizeof(T));
    a0 = v[0];
    a1 = v[1];
  } else {
    a0 = p[0];
    a1 = p[1];
  }
}

// ---------------------------------------------------------------- restriction, fused with the residual
// The workgroup owns coarse cells (ci, cj, ck0 .. ck0 + 255).  Per halved slow axis it reads two fine rows / planes (2 c and
// 2 c + 1; a kept axis: the one of the same index).  Axis 2 halved: lane ck takes the fine cells 2 ck and 2 ck + 1 of each
// row, so consecutive lanes cover one contiguous span of 512 fine cells per row: every byte fetched is used and no fine row
// is read by two workgroups.  Axis 2 kept: every lane loads its own cell of each row.  d = b - q, then the mean along axis
// 2, then axis 1, then axis 0, skipping kept axes.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_restrict_cell(MgBox F, MgBox Cb, int64_t nchunk, const T* __restrict__ b_f,
                                                                const T* __restrict__ q_f, T rscale, T* __restrict__ b_c,
                                                                T* __restrict__ x_c) {
  static_assert(MASK > 0 && MASK < 8, "at least one axis halved");
  constexpr bool H0 = (MASK & 1) != 0, H1 = (MASK & 2) != 0, H2 = (MASK & 4) != 0;
  constexpr int NI = H0 ? 2 : 1, NJ = H1 ? 2 : 1;
  int64_t ci, cj, ck0;
  if (!mg_row(Cb, nchunk, linear_block(), ci, cj, ck0)) return;
  const int64_t ck = ck0 + threadIdx.x;
  if (ck >= Cb.m[2]) return;
  const int64_t fi0 = H0 ? 2 * ci : ci, fj0 = H1 ? 2 * cj : cj, fk = H2 ? 2 * ck : ck;
  T plane[NI];
#pragma unroll
  for (int a = 0; a < NI; ++a) {
    T row[NJ];
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
      const int64_t o = mg_at(F, fi0 + a, fj0 + r, fk);
      if constexpr (H2) {
        // fk is even: the pair's alignment is that of the row's first Omega cell, the same for every lane
        const bool aligned = (((uintptr_t)(b_f + o) | (uintptr_t)(q_f + o)) & (2 * sizeof(T) - 1)) == 0;
        T b0, b1, q0, q1;
        mg_load_pair(b_f + o, aligned, b0, b1);
        mg_load_pair(q_f + o, aligned, q0, q1);
        const T d0 = b0 - q0;
        const T d1 = b1 - q1;
        row[r] = mg_mean(d0, d1);
      } else {
        row[r] = b_f[o] - q_f[o];
      }
    }
    if constexpr (H1) plane[a] = mg_mean(row[0], row[1]);
    else plane[a] = row[0];
  }
  T t;
  if constexpr (H0) t = mg_mean(plane[0], plane[1]);
  else t = plane[0];
  const int64_t oc = mg_at(Cb, ci, cj, ck);
  b_c[oc] = rscale * t;
  x_c[oc] = (T)0;
}

// ---------------------------------------------------------------- prolongation and correction
// The workgroup owns fine cells (fi, fj, fk0 .. fk0 + 255).  The coarse row and plane are workgroup-uniform (fi / 2, fj / 2,
// or the same index on a kept axis); along a halved axis 2 the lanes 2 j and 2 j + 1 read the same coarse cell through L1.
// One coarse operand per fine cell, taken as it is (no operation: -0 and NaN keep their bits), no parity select.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_prolong_add_cell(MgBox F, MgBox Cb, int64_t nchunk, const T* __restrict__ x_c,
                                                                   T* __restrict__ x_f) {
  static_assert(MASK > 0 && MASK < 8, "at least one axis halved");
  int64_t fi, fj, fk0;
  if (!mg_row(F, nchunk, linear_block(), fi, fj, fk0)) return;
  const int64_t fk = fk0 + threadIdx.x;
  if (fk >= F.m[2]) return;
  const int64_t ci = (MASK & 1) ? fi / 2 : fi, cj = (MASK & 2) ? fj / 2 : fj, ck = (MASK & 4) ? fk / 2 : fk;
  const T e = x_c[mg_at(Cb, ci, cj, ck)];
  const int64_t o = mg_at(F, fi, fj, fk);
  x_f[o] = x_f[o] + e;
}

// ================================================================ linear prolongation on a cell-centred pair
// Along a halved axis the fine cell i lies a quarter of a coarse cell from the centre of its own coarse cell j = i / 2,
// towards the neighbour n = j - 1 (even i) or j + 1 (odd i):  p = 0.75 * e[j],  s = 0.25 * v,  t = p + s  with v = e[n], or,
// where n is outside the coarse Omega, the ghost value the face's rule gives: +e[j] (EVEN: a Neumann face) or -e[j] (ODD:
// the value 0 on the face).  e is the intermediate after the axes already done (axis 2, then 1, then 0), so a ghost along a
// later axis is +- the intermediate at the edge.  The negation is a sign flip: exact, and 0.25 * (-a) = -(0.25 * a).

// the rule per face on the kernels' three axes: 0 = EVEN, 1 = ODD; axes that are kept are never looked at
struct MgRim {
  int32_t lo[3], hi[3];
};
template <class T>
__device__ __forceinline__ T mg_lin(T own, T v) {
  const T p = (T)0.75 * own;
  const T s = (T)0.25 * v;
  return p + s;
}
// the coarse indices one fine index needs along one axis: its own cell, and the neighbour -- or, where that is outside
// [0, m_c), `ghost`, with `near` = own (always a cell of Omega) and `flip` = the face's rule is ODD.  A kept axis: own only.
struct MgNear {
  int64_t own, near;
  bool ghost, flip;
};
__device__ __forceinline__ MgNear mg_near(bool halved, int64_t i, int64_t m_c, int32_t rule_lo, int32_t rule_hi) {
  MgNear s;
  s.own = halved ? i / 2 : i;
  const int64_t n = (i & 1) ? s.own + 1 : s.own - 1;
  s.ghost = halved && (n < 0 || n >= m_c);
  s.flip = s.ghost && (n < 0 ? rule_lo : rule_hi) != 0;
  s.near = (halved && !s.ghost) ? n : s.own;
  return s;
}
template <class T>
__device__ __forceinline__ void mg_store_pair(T* p, bool aligned, T a0, T a1) {
  if (aligned) {
    const T v[2] = {a0, a1};
    __builtin_memcpy(__builtin_assume_aligned(p, 2 * sizeof(T)), v, 2 * sizeof(T));
  } else {
    p[0] = a0;
    p[1] = a1;
  }
}

// The workgroup owns one chunk of the fine row (fi, fj).  Along axes 0 and 1 the own and the neighbour coarse row / plane,
// and whether the neighbour is a ghost, are workgroup-uniform scalar work (mg_near); a ghost row is not loaded at all: it
// is +- the intermediate of the own row.  Up to 2 x 2 coarse rows feed a fine row, all through L1 / L2 -- the coarse field is
// 1 / 2^k of the fine one.  Along axis 2:
//   halved (PAIR): the workgroup's chunk is 256 COARSE cells; the lane owns the coarse index ck and the fine cells 2 ck,
//     2 ck + 1, formed from e[ck - 1], e[ck], e[ck + 1] of each coarse row (three coalesced loads; the product 0.75 * e[ck]
//     is the same value for both cells); x_f is read and written as one access of 2 sizeof(T) where the row's first Omega
//     cell is aligned to that, as two otherwise -- the same bits.  Only lanes ck = 0 and ck = m - 1 meet a ghost: a per-lane
//     select.  (A form with one fine cell per lane, two coarse loads by parity, measured 1.6x slower: DESIGN 3.22.)
//   kept: the chunk is 256 fine cells, the lane loads e[fk] alone.
// A neighbour index outside the coarse Omega is clamped to the own cell before the load, so no coarse cell outside Omega is
// read; no fine cell outside Omega is written.  No LDS, no barrier, no atomics.
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_prolong_add_linear(MgBox F, MgBox Cb, int64_t nchunk, MgRim rim,
                                                                     const T* __restrict__ x_c, T* __restrict__ x_f) {
  static_assert(MASK > 0 && MASK < 8, "at least one axis halved");
  constexpr bool H0 = (MASK & 1) != 0, H1 = (MASK & 2) != 0, PAIR = (MASK & 4) != 0;
  constexpr int NI = H0 ? 2 : 1, NJ = H1 ? 2 : 1, W = PAIR ? 2 : 1;
  int64_t fi, fj, k0;
  if (!mg_row(F, nchunk, linear_block(), fi, fj, k0)) return;
  const int64_t k = k0 + threadIdx.x;   // PAIR: the coarse interior index along axis 2; else the fine one
  if (k >= (PAIR ? Cb.m[2] : F.m[2])) return;
  const MgNear si = mg_near(H0, fi, Cb.m[0], rim.lo[0], rim.hi[0]);
  const MgNear sj = mg_near(H1, fj, Cb.m[1], rim.lo[1], rim.hi[1]);
  const int64_t ci[2] = {si.own, si.near}, cj[2] = {sj.own, sj.near};
  T ei[NI][W];
#pragma unroll
  for (int a = 0; a < NI; ++a) {
    if (a == 1 && si.ghost) {
#pragma unroll
      for (int w = 0; w < W; ++w) ei[a][w] = si.flip ? -ei[0][w] : ei[0][w];
      continue;
    }
    T ej[NJ][W];
#pragma unroll
    for (int r = 0; r < NJ; ++r) {
      if (r == 1 && sj.ghost) {
#pragma unroll
        for (int w = 0; w < W; ++w) ej[r][w] = sj.flip ? -ej[0][w] : ej[0][w];
        continue;
      }
      const T* row = x_c + mg_at(Cb, ci[a], cj[r], 0);
      if constexpr (PAIR) {
        const bool first = k == 0, last = k + 1 == Cb.m[2];
        const T own = row[k];
        T vm = row[first ? k : k - 1];
        T vp = row[last ? k : k + 1];
        if (first && rim.lo[2] != 0) vm = -vm;
        if (last && rim.hi[2] != 0) vp = -vp;
        const T p = (T)0.75 * own;
        const T sm = (T)0.25 * vm;
        const T sp = (T)0.25 * vp;
        ej[r][0] = p + sm;
        ej[r][1] = p + sp;
      } else {
        ej[r][0] = row[k];
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if constexpr (H1) ei[a][w] = mg_lin(ej[0][w], ej[1][w]);
      else ei[a][w] = ej[0][w];
    }
  }
  T e[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    if constexpr (H0) e[w] = mg_lin(ei[0][w], ei[1][w]);
    else e[w] = ei[0][w];
  }
  if constexpr (PAIR) {
    // 2 k is even: the pair's alignment is that of the row's first Omega cell, the same for every lane
    T* const p = x_f + mg_at(F, fi, fj, 2 * k);
    const bool aligned = ((uintptr_t)p & (2 * sizeof(T) - 1)) == 0;
    T a0, a1;
    mg_load_pair(p, aligned, a0, a1);
    const T u0 = a0 + e[0];
    const T u1 = a1 + e[1];
    mg_store_pair(p, aligned, u0, u1);
  } else {
    const int64_t o = mg_at(F, fi, fj, k);
    x_f[o] = x_f[o] + e[0];
  }
}

// ================================================================ transposed linear restriction on a cell-centred pair
// R = P^T / 2 per halved axis, P the linear prolongation above with the same rule per face.  Along a halved axis the coarse
// cell j takes the four fine values a[2 j - 1 .. 2 j + 2] with the weights 1/4, 3/4, 3/4, 1/4 and half of their sum; an outer
// operand outside the fine Omega is the ghost +a[edge] (EVEN) or -a[edge] (ODD) -- padding the fine array with +- its edge is
// the transpose of padding the coarse one.  a is the intermediate after the axes already done (axis 2, then 1, then 0).
template <class T>
__device__ __forceinline__ T mg_lin4(T am, T a0, T a1, T ap) {
  const T sm = (T)0.25 * am;
  const T p0 = (T)0.75 * a0;
  const T p1 = (T)0.75 * a1;
  const T sp = (T)0.25 * ap;
  const T u = sm + p0;
  const T v = p1 + sp;
  const T w = u + v;
  return (T)0.5 * w;
}
// The lane's value of ONE fine row after axis 2; b_row, q_row: the row's first Omega cell.  Called by all 256 lanes together.
//   halved: the lane owns the coarse index ck, loads the pair d[2 ck], d[2 ck + 1] (d = b - q; one access of 2 sizeof(T) where
//     the row is aligned to that, workgroup-uniform) and takes d[2 ck - 1], d[2 ck + 2] from the neighbouring lanes' pairs by
//     a wave shift; lane 0 and lane 63 of a wave load their one extra cell (`edge` of the shift).  The lanes ck = 0 and
//     ck = m_c - 1 take the ghost instead: a per-lane select.  A lane without a cell (ck >= m_c) loads nothing.
//   kept: d[ck] itself.
template <class T, bool H2>
__device__ __forceinline__ T mg_lin_row(const T* __restrict__ b_row, const T* __restrict__ q_row, int64_t ck, int64_t m_c, bool owns,
                                        int lane, int32_t rule_lo, int32_t rule_hi) {
  if constexpr (!H2) {
    return owns ? b_row[ck] - q_row[ck] : (T)0;
  } else {
    const bool aligned = (((uintptr_t)b_row | (uintptr_t)q_row) & (2 * sizeof(T) - 1)) == 0;
    const bool first = ck == 0, last = ck + 1 == m_c;
    T d0 = (T)0, d1 = (T)0, em = (T)0, ep = (T)0;
    if (owns) {
      T b0, b1, q0, q1;
      mg_load_pair(b_row + 2 * ck, aligned, b0, b1);
      mg_load_pair(q_row + 2 * ck, aligned, q0, q1);
      d0 = b0 - q0;
      d1 = b1 - q1;
      if (lane == 0 && !first) em = b_row[2 * ck - 1] - q_row[2 * ck - 1];
      if (lane == kWave - 1 && !last) ep = b_row[2 * ck + 2] - q_row[2 * ck + 2];
    }
    T am = from_prev<true>(d1, em, lane);
    T ap = from_next<true>(d0, ep, lane);
    if (first) am = rule_lo != 0 ? -d0 : d0;
    if (last) ap = rule_hi != 0 ? -d1 : d1;
    return mg_lin4(am, d0, d1, ap);
  }
}

// The workgroup owns one 256-cell chunk along axis 2 of the coarse plane ci and MARCHES a run of kMgLinearRun coarse rows
// along axis 1.  Axis 1 halved: coarse row cj needs the fine rows 2 cj - 1 .. 2 cj + 2, of which two were the previous step's;
// per fine plane the last four axis-2 results stay in registers (ring), so a step loads two new fine rows per plane and a
// fine row is loaded once per workgroup along that axis (twice where two runs meet).  Axis 0 halved: the four fine planes
// 2 ci - 1 .. 2 ci + 2 are read directly, each carrying its own ring; the two coarse planes that share a fine plane fetch it
// twice unless a cache holds it (the pass model is in DESIGN 3.23).  A ghost row or plane is never loaded: it is +- the
// intermediate of the edge row / plane, workgroup-uniform scalar work.  No fine cell outside Omega is read, no coarse cell
// outside Omega is written.  No LDS, no barrier, no atomics; every lane stays in the loop (the wave shifts need them all).
constexpr int kMgLinearRun = 8;
template <class T, int MASK>
__global__ __launch_bounds__(256) void neptune_mg_restrict_linear(MgBox F, MgBox Cb, int64_t nchunk, MgRim rim, const T* __restrict__ b_f,
                                                                  const T* __restrict__ q_f, T rscale, T* __restrict__ b_c,
                                                                  T* __restrict__ x_c) {
  static_assert(MASK > 0 && MASK < 8, "at least one axis halved");
  constexpr bool H0 = (MASK & 1) != 0, H1 = (MASK & 2) != 0, H2 = (MASK & 4) != 0;
  constexpr int NI = H0 ? 4 : 1, NJ = H1 ? 4 : 1;
  const int64_t nrun = (Cb.m[1] + kMgLinearRun - 1) / kMgLinearRun;
  const int64_t blk = linear_block();
  if (blk >= Cb.m[0] * nrun * nchunk) return;   // workgroup-uniform
  const int64_t pr = blk / nchunk, c = blk - pr * nchunk;
  const int64_t ci = pr / nrun, cj0 = (pr - ci * nrun) * kMgLinearRun;
  const int64_t cj1 = cj0 + kMgLinearRun < Cb.m[1] ? cj0 + kMgLinearRun : Cb.m[1];
  const int64_t ck = c * 256 + threadIdx.x;
  const bool owns = ck < Cb.m[2];
  const int lane = threadIdx.x & (kWave - 1);
  // plane a of the NI is the fine plane fi0 + a; the outer ones are ghosts on the first / last coarse plane
  const bool glo0 = H0 && ci == 0, ghi0 = H0 && ci + 1 == Cb.m[0];
  const int64_t fi0 = H0 ? 2 * ci - 1 : ci;
  auto row = [&](int64_t fi, int64_t fj) {
    const int64_t o = mg_at(F, fi, fj, 0);
    return mg_lin_row<T, H2>(b_f + o, q_f + o, ck, Cb.m[2], owns, lane, rim.lo[2], rim.hi[2]);
  };
  T ring[NI][NJ];
  for (int64_t cj = cj0; cj < cj1; ++cj) {
    const bool glo1 = H1 && cj == 0, ghi1 = H1 && cj + 1 == Cb.m[1];
    const int64_t fj0 = H1 ? 2 * cj - 1 : cj;   // slot r of the ring is the fine row fj0 + r
    T pa[NI];
#pragma unroll
    for (int a = 0; a < NI; ++a) {
      if ((a == 0 && glo0) || (a == NI - 1 && ghi0)) continue;
      if constexpr (H1) {
        if (cj == cj0) {
          if (!glo1) ring[a][0] = row(fi0 + a, fj0);
          ring[a][1] = row(fi0 + a, fj0 + 1);
        } else {
          ring[a][0] = ring[a][2];
          ring[a][1] = ring[a][3];
        }
        ring[a][2] = row(fi0 + a, fj0 + 2);
        if (!ghi1) ring[a][3] = row(fi0 + a, fj0 + 3);
        if (glo1) ring[a][0] = rim.lo[1] != 0 ? -ring[a][1] : ring[a][1];
        if (ghi1) ring[a][3] = rim.hi[1] != 0 ? -ring[a][2] : ring[a][2];
        pa[a] = mg_lin4(ring[a][0], ring[a][1], ring[a][2], ring[a][3]);
      } else {
        pa[a] = row(fi0 + a, fj0);
      }
    }
    T t;
    if constexpr (H0) {
      if (glo0) pa[0] = rim.lo[0] != 0 ? -pa[1] : pa[1];
      if (ghi0) pa[3] = rim.hi[0] != 0 ? -pa[2] : pa[2];
      t = mg_lin4(pa[0], pa[1], pa[2], pa[3]);
    } else {
      t = pa[0];
    }
    if (owns) {
      const int64_t oc = mg_at(Cb, ci, cj, ck);
      b_c[oc] = rscale * t;
      x_c[oc] = (T)0;
    }
  }
}

}  // namespace neptune_hip
