// mg_line_kernels.hpp -- the line smoother's kernels (neptune_hip_mg_line_smooth): one stage of a line-Jacobi
// sweep, a batched tridiagonal solve along one axis of Omega from the factors lo, inv, up of Thomas's elimination.
//
//   neptune_mg_line_slow     lines along box axis 0 or 1: one lane per line, lanes along the contiguous axis
//   neptune_mg_line_contig   lines along box axis 2 (the contiguous one): a wave owns 64 lines and walks them in segments
//                            that are transposed through LDS
//
// Per line of Omega along the axis (interior index i, m cells), from q = A(x) of the plain launch just before:
//   forward    d_i = b_i - q_i;  g_0 = d_0 * inv_0;  i >= 1:  t = lo_i * g_(i-1),  s = d_i - t,  g_i = s * inv_i     (g is stored into q)
//   backward   e_(m-1) = g_(m-1);  i < m-1:  t = up_i * e_(i+1),  e_i = g_i - t
//   update     x_i = x_i + e_i
// lo_0 and up_(m-1) are never read.  The values are those of these recurrences: the solve along a line is sequential.
// Passes: reads q, b, lo, inv, writes g; reads g, up, x, writes x: 8.
//
// The frame is multigrid_kernels.hpp's: MgBox on three right-aligned axes, only Omega's cells are ever addressed, everything
// in T with every intermediate a named temporary and one rounding per operation (-ffp-contract=off), no atomics, no
// reductions.  Templates only: multigrid.hip instantiates them.
#pragma once
#include "multigrid_kernels.hpp"

namespace neptune_hip {

// ---------------------------------------------------------------- lines along a slow axis
// A workgroup owns WIDTH consecutive cells along axis 2 at one interior index `o` of the OTHER slow axis; each lane owns the
// line through its cell and marches i upward, then downward.  Consecutive lanes sit on consecutive addresses at every step,
// so every global access is coalesced.  No address depends on the recurrence: the loads of kMgLineUnroll steps are issued
// together ahead of the dependent multiply - subtract - multiply chain, which is the latency floor of a line.  The lane that
// stored g_i reads it back itself on the way down: no barrier, no other lane's data.
// WIDTH is 256, or 64 where the level has too few lines to fill the CUs with 256-lane workgroups (the host decides).
constexpr int kMgLineUnroll = 4;

template <class T, int AXIS, int WIDTH>
__global__ __launch_bounds__(WIDTH) void neptune_mg_line_slow(MgBox B, int64_t nchunk, T* __restrict__ q, const T* __restrict__ b,
                                                              const T* __restrict__ lo, const T* __restrict__ inv,
                                                              const T* __restrict__ up, T* __restrict__ x) {
  static_assert(AXIS == 0 || AXIS == 1, "a slow axis");
  constexpr int OTHER = 1 - AXIS;
  constexpr int U = kMgLineUnroll;
  const int64_t blk = linear_block();
  if (blk >= B.m[OTHER] * nchunk) return;
  const int64_t o = blk / nchunk, c = blk - o * nchunk;
  const int64_t k = c * WIDTH + threadIdx.x;
  if (k >= B.m[2]) return;
  const int64_t first = AXIS == 0 ? mg_at(B, 0, o, k) : mg_at(B, o, 0, k);
  const int64_t step = AXIS == 0 ? B.n[1] * B.n[2] : B.n[2];
  const int64_t m = B.m[AXIS];

  // ---- forward: g into q
  T g;
  {
    const T d = b[first] - q[first];
    g = d * inv[first];
    q[first] = g;
  }
  int64_t i = 1;
  for (; i + U <= m; i += U) {
    T dv[U], lv[U], iv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = first + (i + u) * step;
      const T bb = b[off];
      const T qq = q[off];
      lv[u] = lo[off];
      iv[u] = inv[off];
      dv[u] = bb - qq;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T t = lv[u] * g;
      const T s = dv[u] - t;
      g = s * iv[u];
      q[first + (i + u) * step] = g;
    }
  }
  for (; i < m; ++i) {
    const int64_t off = first + i * step;
    const T d = b[off] - q[off];
    const T t = lo[off] * g;
    const T s = d - t;
    g = s * inv[off];
    q[off] = g;
  }

  // ---- backward and update
  T e = g;
  {
    const int64_t off = first + (m - 1) * step;
    x[off] = x[off] + e;
  }
  i = m - 2;
  for (; i - (U - 1) >= 0; i -= U) {
    T uv[U], gv[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = first + (i - u) * step;
      uv[u] = up[off];
      gv[u] = q[off];
      xv[u] = x[off];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T t = uv[u] * e;
      e = gv[u] - t;
      x[first + (i - u) * step] = xv[u] + e;
    }
  }
  for (; i >= 0; --i) {
    const int64_t off = first + i * step;
    const T t = up[off] * e;
    e = q[off] - t;
    x[off] = x[off] + e;
  }
}

// ---------------------------------------------------------------- lines along the contiguous axis
// One lane per line straight from memory would stride by a whole row.  Instead a workgroup of ONE wave owns kMgLineGroup = 64
// consecutive lines (rows of Omega in row-major order of axes 0, 1) and walks them in segments of kMgLineSeg cells:
//   stage   the two 32-lane halves of the wave each take one line per round, lanes along the line: b - q, lo, inv of the
//           segment (backward: g, up, x) are loaded coalesced -- 32 consecutive cells, 256 B of f64 -- and stored to three LDS
//           arrays [line][cell] of pitch kMgLinePitch;
//   solve   lane r runs the recurrence over line r's cells out of LDS, carrying g_(i-1) (backward: e_(i+1)) in a register
//           from one segment to the next, and leaves g (backward: x + e) in place;
//   store   g (backward: x) goes back the way it came, coalesced.
// The pitch is odd: in the solve phase lane r addresses r * pitch + cell, so the 32 lanes of a half-wave fall on 32 distinct
// banks (f32) or bank pairs (f64); in the stage and store phases the lanes of a half-wave address consecutive cells.
// Sizes.  The stage phase is what the kernel waits for (the solve phase is a few hundred cycles per segment), so the segment
// only has to keep enough bytes in flight per CU: 32 cells x 64 lines x 4 arrays = 64 KiB of f64 loads per wave and segment.
// LDS is 3 x 64 x 33 elements = 50,688 B (f64) / 25,344 B (f32) plus the 512-B table of the lines' offsets: 3 (f64) or 6 (f32)
// workgroups fit the 160 KiB of a CU, each a wave with its own segment in flight.  A longer segment would halve that
// occupancy for nothing, a shorter one would cut the coalesced runs below two 128-B lines.  One wave per workgroup keeps
// the barriers wave-local.  With so few waves per CU the bytes in flight have to come from each wave: the stage phase loads
// kMgLineRounds = 16 rounds -- 64 loads of 512 B (f64) -- into registers before the first of them is stored to LDS (a plain
// unrolled load - store loop waits for every round's loads in turn).  The lo (up) of the one cell that is never read is
// not loaded: that lane stages +0 in its place.
constexpr int kMgLineGroup = 64;
constexpr int kMgLineSeg = 32;
constexpr int kMgLinePitch = kMgLineSeg + 1;
constexpr int kMgLineRounds = 16;   // rounds of the stage phase whose loads are issued together

template <class T>
__global__ __launch_bounds__(kMgLineGroup) void neptune_mg_line_contig(MgBox B, T* __restrict__ q, const T* __restrict__ b,
                                                                       const T* __restrict__ lo, const T* __restrict__ inv,
                                                                       const T* __restrict__ up, T* __restrict__ x) {
  constexpr int SEG = kMgLineSeg, P = kMgLinePitch, R = kMgLineRounds;
  __shared__ T s0[kMgLineGroup * P];   // forward: d, then g; backward: g
  __shared__ T s1[kMgLineGroup * P];   // forward: lo; backward: up
  __shared__ T s2[kMgLineGroup * P];   // forward: inv; backward: x, then x + e
  __shared__ int64_t sbase[kMgLineGroup];
  const int lane = threadIdx.x;
  const int64_t nlines = B.m[0] * B.m[1];
  const int64_t line0 = linear_block() * kMgLineGroup;
  if (line0 >= nlines) return;   // workgroup-uniform: past the last workgroup of a folded grid
  const int64_t rest = nlines - line0;
  const int nvalid = (int)(rest < (int64_t)kMgLineGroup ? rest : (int64_t)kMgLineGroup);
  const bool owns = lane < nvalid;
  {
    const int64_t mine = line0 + (owns ? lane : 0);
    const int64_t li = mine / B.m[1], lj = mine - li * B.m[1];
    sbase[lane] = mg_at(B, li, lj, 0);
  }
  __syncthreads();
  const int64_t m = B.m[2];
  const int c = lane & (SEG - 1), half = lane >> 5;
  static_assert(SEG == 32 && kMgLineGroup == 64, "two half-waves, one line each per round");
  T* const r0 = s0 + lane * P;
  T* const r1 = s1 + lane * P;
  T* const r2 = s2 + lane * P;

  // ---- forward: g into q
  T carry = (T)0;
  for (int64_t seg0 = 0; seg0 < m; seg0 += SEG) {
    const int len = (int)(m - seg0 < (int64_t)SEG ? m - seg0 : (int64_t)SEG);
    if (c < len) {
      const bool reads_lo = seg0 + c > 0;   // lo_0 is never read
      for (int r0 = half; r0 < nvalid; r0 += 2 * R) {
        T bv[R], qv[R], iv[R], lv[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int r = r0 + 2 * j < nvalid ? r0 + 2 * j : nvalid - 1;   // past the group's tail: a line of the group again
          const int64_t off = sbase[r] + seg0 + c;
          bv[j] = b[off];
          qv[j] = q[off];
          iv[j] = inv[off];
          lv[j] = reads_lo ? lo[off] : (T)0;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int r = r0 + 2 * j;
          if (r < nvalid) {
            const int at = r * P + c;
            const T d = bv[j] - qv[j];
            s0[at] = d;
            s1[at] = lv[j];
            s2[at] = iv[j];
          }
        }
      }
    }
    __syncthreads();
    if (owns) {
      int cc = 0;
      T g = carry;
      if (seg0 == 0) {
        const T d = r0[0];
        g = d * r2[0];
        r0[0] = g;
        cc = 1;
      }
      for (; cc < len; ++cc) {
        const T t = r1[cc] * g;
        const T s = r0[cc] - t;
        g = s * r2[cc];
        r0[cc] = g;
      }
      carry = g;
    }
    __syncthreads();
    if (c < len) {
#pragma unroll 4
      for (int r = half; r < nvalid; r += 2) q[sbase[r] + seg0 + c] = s0[r * P + c];
    }
    __syncthreads();
  }

  // ---- backward and update, from the far end; `carry` becomes e_(i+1)
  for (int64_t seg0 = ((m - 1) / SEG) * SEG; seg0 >= 0; seg0 -= SEG) {
    const int len = (int)(m - seg0 < (int64_t)SEG ? m - seg0 : (int64_t)SEG);
    if (c < len) {
      const bool reads_up = seg0 + c < m - 1;   // up_(m-1) is never read
      for (int r0 = half; r0 < nvalid; r0 += 2 * R) {
        T gv[R], xv[R], uv[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int r = r0 + 2 * j < nvalid ? r0 + 2 * j : nvalid - 1;
          const int64_t off = sbase[r] + seg0 + c;
          gv[j] = q[off];
          xv[j] = x[off];
          uv[j] = reads_up ? up[off] : (T)0;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int r = r0 + 2 * j;
          if (r < nvalid) {
            const int at = r * P + c;
            s0[at] = gv[j];
            s1[at] = uv[j];
            s2[at] = xv[j];
          }
        }
      }
    }
    __syncthreads();
    if (owns) {
      int cc = len - 1;
      T e = carry;
      if (seg0 + len == m) {
        e = r0[cc];
        r2[cc] = r2[cc] + e;
        --cc;
      }
      for (; cc >= 0; --cc) {
        const T t = r1[cc] * e;
        e = r0[cc] - t;
        r2[cc] = r2[cc] + e;
      }
      carry = e;
    }
    __syncthreads();
    if (c < len) {
#pragma unroll 4
      for (int r = half; r < nvalid; r += 2) x[sbase[r] + seg0 + c] = s2[r * P + c];
    }
    __syncthreads();
  }
}

}  // namespace neptune_hip
