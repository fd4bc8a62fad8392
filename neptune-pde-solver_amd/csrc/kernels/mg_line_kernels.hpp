// mg_line_kernels.hpp -- the line smoother's kernels (neptune_hip_mg_line_smooth): one stage of a line-Jacobi
// sweep, a batched tridiagonal solve along one axis of Omega from the factors lo, inv, up of Thomas's elimination.
//
//   neptune_mg_line_slow     lines along box axis 0 or 1: one lane per line, lanes along the contiguous axis
//   neptune_mg_line_contig   lines along box axis 2 (the contiguous one): a wave owns 64 lines and walks them in segments
//                            that are transposed through LDS
//
//   neptune_mg_line_{slow,contig}_first   the apply-free form of either: the stage on q = +0, x = +0
//   neptune_mg_line_{slow,contig}_dot     either with the sum of b * x_new out of the backward march
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

// The stage's three forms.  kMgLinePlain is the stage as above.  kMgLineFirst is the stage on q = +0, x = +0
// without reading either: d_i = b_i, g is kept in x (q is not touched), x_i = (+0) + e_i -- the addition stays, it turns a
// -0 into the +0 of the plain stage.  kMgLineDot is the plain stage that also forms t_i = b_i * x_new,i in the backward
// march, one rounding, and adds it to the lane's accumulator in the order of that march (i = m-1 .. 0) from +0.
enum : int { kMgLinePlain = 0, kMgLineFirst = 1, kMgLineDot = 2 };

// -> the lane's accumulator (kMgLineDot; +0 otherwise and for a lane without a line)
template <class T, int AXIS, int WIDTH, int MODE>
__device__ __forceinline__ T mg_line_slow_body(const MgBox& B, int64_t nchunk, T* __restrict__ q, const T* __restrict__ b,
                                               const T* __restrict__ lo, const T* __restrict__ inv, const T* __restrict__ up,
                                               T* __restrict__ x) {
  static_assert(AXIS == 0 || AXIS == 1, "a slow axis");
  constexpr int OTHER = 1 - AXIS;
  constexpr int U = kMgLineUnroll;
  constexpr bool FIRST = MODE == kMgLineFirst, DOT = MODE == kMgLineDot;
  T acc = (T)0;
  T* const gq = FIRST ? x : q;   // where g is kept between the two marches
  const T zero = (T)0;
  const int64_t blk = linear_block();
  if (blk >= B.m[OTHER] * nchunk) return acc;
  const int64_t o = blk / nchunk, c = blk - o * nchunk;
  const int64_t k = c * WIDTH + threadIdx.x;
  if (k >= B.m[2]) return acc;
  const int64_t first = AXIS == 0 ? mg_at(B, 0, o, k) : mg_at(B, o, 0, k);
  const int64_t step = AXIS == 0 ? B.n[1] * B.n[2] : B.n[2];
  const int64_t m = B.m[AXIS];

  // ---- forward: g into q
  // d of one cell: b - q, or b itself
  auto rhs = [&](int64_t off) -> T {
    const T bb = b[off];
    if constexpr (FIRST) {
      return bb;
    } else {
      const T qq = q[off];
      return bb - qq;
    }
  };
  T g;
  {
    const T d = rhs(first);
    g = d * inv[first];
    gq[first] = g;
  }
  int64_t i = 1;
  for (; i + U <= m; i += U) {
    T dv[U], lv[U], iv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = first + (i + u) * step;
      dv[u] = rhs(off);
      lv[u] = lo[off];
      iv[u] = inv[off];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T t = lv[u] * g;
      const T s = dv[u] - t;
      g = s * iv[u];
      gq[first + (i + u) * step] = g;
    }
  }
  for (; i < m; ++i) {
    const int64_t off = first + i * step;
    const T d = rhs(off);
    const T t = lo[off] * g;
    const T s = d - t;
    g = s * inv[off];
    gq[off] = g;
  }

  // ---- backward and update
  // x_new of one cell from its e (and, kMgLineDot, its term of b . x_new into the accumulator)
  auto update = [&](int64_t off, T xv, T bv, T e) {
    const T xn = xv + e;
    x[off] = xn;
    if constexpr (DOT) {
      const T t = bv * xn;
      acc += t;
    }
  };
  T e = g;
  {
    const int64_t off = first + (m - 1) * step;
    update(off, FIRST ? zero : x[off], DOT ? b[off] : zero, e);
  }
  i = m - 2;
  for (; i - (U - 1) >= 0; i -= U) {
    T uv[U], gv[U], xv[U], bv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = first + (i - u) * step;
      uv[u] = up[off];
      gv[u] = gq[off];
      xv[u] = FIRST ? zero : x[off];
      bv[u] = DOT ? b[off] : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T t = uv[u] * e;
      e = gv[u] - t;
      update(first + (i - u) * step, xv[u], bv[u], e);
    }
  }
  for (; i >= 0; --i) {
    const int64_t off = first + i * step;
    const T t = up[off] * e;
    e = gq[off] - t;
    update(off, FIRST ? zero : x[off], DOT ? b[off] : zero, e);
  }
  return acc;
}

template <class T, int AXIS, int WIDTH>
__global__ __launch_bounds__(WIDTH) void neptune_mg_line_slow(MgBox B, int64_t nchunk, T* __restrict__ q, const T* __restrict__ b,
                                                              const T* __restrict__ lo, const T* __restrict__ inv,
                                                              const T* __restrict__ up, T* __restrict__ x) {
  (void)mg_line_slow_body<T, AXIS, WIDTH, kMgLinePlain>(B, nchunk, q, b, lo, inv, up, x);
}
// the apply-free stage: reads b, lo, inv, up, writes x on Omega (g on the way up, x on the way down): 7 passes
template <class T, int AXIS, int WIDTH>
__global__ __launch_bounds__(WIDTH) void neptune_mg_line_slow_first(MgBox B, int64_t nchunk, const T* __restrict__ b,
                                                                    const T* __restrict__ lo, const T* __restrict__ inv,
                                                                    const T* __restrict__ up, T* __restrict__ x) {
  (void)mg_line_slow_body<T, AXIS, WIDTH, kMgLineFirst>(B, nchunk, (T*)nullptr, b, lo, inv, up, x);
}
// the stage with b . x_new: the backward march also loads b, 9 passes; one partial per workgroup of the (possibly folded)
// grid at its linear index -- the lanes' accumulators on the tree of the monitored launches (monitor_block_sum)
template <class T, int AXIS, int WIDTH>
__global__ __launch_bounds__(WIDTH) void neptune_mg_line_slow_dot(MgBox B, int64_t nchunk, T* __restrict__ q, const T* __restrict__ b,
                                                                  const T* __restrict__ lo, const T* __restrict__ inv,
                                                                  const T* __restrict__ up, T* __restrict__ x,
                                                                  T* __restrict__ partials) {
  __shared__ T lds[4];
  const T acc = mg_line_slow_body<T, AXIS, WIDTH, kMgLineDot>(B, nchunk, q, b, lo, inv, up, x);
  const T sum = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[linear_block()] = sum;
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

// The three forms as for the slow axes.  kMgLineFirst stages b, lo, inv on the way up (d = b), keeps g in x, and on the way
// down stages two arrays, g and up: the result (+0) + e replaces g in place.  kMgLineDot needs b beside g, up, x on the way
// down: its loads are issued with the others and held in registers over the solve phase, then staged through the array of
// up, which that phase has consumed; lane r adds line r's terms b * x_new out of LDS in the order of the backward march.  No
// fourth array.  -> the lane's accumulator (kMgLineDot; +0 otherwise)
template <class T, int MODE>
__device__ __forceinline__ T mg_line_contig_body(const MgBox& B, T* __restrict__ q, const T* __restrict__ b, const T* __restrict__ lo,
                                                 const T* __restrict__ inv, const T* __restrict__ up, T* __restrict__ x) {
  constexpr int SEG = kMgLineSeg, P = kMgLinePitch, R = kMgLineRounds;
  constexpr bool FIRST = MODE == kMgLineFirst, DOT = MODE == kMgLineDot;
  constexpr int BATCHES = kMgLineGroup / (2 * R);   // batches of R rounds that cover the group's lines
  __shared__ T s0[kMgLineGroup * P];   // forward: d, then g; backward: g (kMgLineFirst: then (+0) + e)
  __shared__ T s1[kMgLineGroup * P];   // forward: lo; backward: up (kMgLineDot: then b)
  __shared__ T s2[kMgLineGroup * P];   // forward: inv; backward: x, then x + e (kMgLineFirst: unused)
  __shared__ int64_t sbase[kMgLineGroup];
  T acc = (T)0;
  T* const gq = FIRST ? x : q;         // where g is kept between the two marches
  const int lane = threadIdx.x;
  const int64_t nlines = B.m[0] * B.m[1];
  const int64_t line0 = linear_block() * kMgLineGroup;
  if (line0 >= nlines) return acc;   // workgroup-uniform: past the last workgroup of a folded grid
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

  // ---- forward: g into q (kMgLineFirst: into x)
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
          if constexpr (!FIRST) qv[j] = q[off];
          iv[j] = inv[off];
          lv[j] = reads_lo ? lo[off] : (T)0;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int r = r0 + 2 * j;
          if (r < nvalid) {
            const int at = r * P + c;
            T d = bv[j];
            if constexpr (!FIRST) d = bv[j] - qv[j];
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
      for (int r = half; r < nvalid; r += 2) gq[sbase[r] + seg0 + c] = s0[r * P + c];
    }
    __syncthreads();
  }

  // ---- backward and update, from the far end; `carry` becomes e_(i+1)
  const T zero = (T)0;
  for (int64_t seg0 = ((m - 1) / SEG) * SEG; seg0 >= 0; seg0 -= SEG) {
    const int len = (int)(m - seg0 < (int64_t)SEG ? m - seg0 : (int64_t)SEG);
    [[maybe_unused]] T bh[DOT ? BATCHES : 1][DOT ? R : 1];   // kMgLineDot: b of this lane's cells, held over the solve phase
    if (c < len) {
      const bool reads_up = seg0 + c < m - 1;   // up_(m-1) is never read
      if constexpr (DOT) {
#pragma unroll
        for (int bt = 0; bt < BATCHES; ++bt) {
          const int r0 = half + bt * 2 * R;
          if (r0 < nvalid) {
            T gv[R], xv[R], uv[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
              const int r = r0 + 2 * j < nvalid ? r0 + 2 * j : nvalid - 1;
              const int64_t off = sbase[r] + seg0 + c;
              gv[j] = q[off];
              xv[j] = x[off];
              uv[j] = reads_up ? up[off] : (T)0;
              bh[bt][j] = b[off];
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
      } else {
        for (int r0 = half; r0 < nvalid; r0 += 2 * R) {
          T gv[R], xv[R], uv[R];
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const int r = r0 + 2 * j < nvalid ? r0 + 2 * j : nvalid - 1;
            const int64_t off = sbase[r] + seg0 + c;
            gv[j] = gq[off];
            if constexpr (!FIRST) xv[j] = x[off];
            uv[j] = reads_up ? up[off] : (T)0;
          }
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const int r = r0 + 2 * j;
            if (r < nvalid) {
              const int at = r * P + c;
              s0[at] = gv[j];
              s1[at] = uv[j];
              if constexpr (!FIRST) s2[at] = xv[j];
            }
          }
        }
      }
    }
    __syncthreads();
    T* const rx = FIRST ? r0 : r2;   // the line's x: kMgLineFirst leaves (+0) + e where g was
    if (owns) {
      int cc = len - 1;
      T e = carry;
      if (seg0 + len == m) {
        e = r0[cc];
        rx[cc] = (FIRST ? zero : r2[cc]) + e;
        --cc;
      }
      for (; cc >= 0; --cc) {
        const T t = r1[cc] * e;
        e = r0[cc] - t;
        rx[cc] = (FIRST ? zero : r2[cc]) + e;
      }
      carry = e;
    }
    __syncthreads();
    if constexpr (DOT) {
      // up is consumed: b goes through its array, then lane r adds line r's terms from the segment's far end down
      if (c < len) {
#pragma unroll
        for (int bt = 0; bt < BATCHES; ++bt) {
          const int r0 = half + bt * 2 * R;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const int r = r0 + 2 * j;
            if (r < nvalid) s1[r * P + c] = bh[bt][j];
          }
        }
      }
      __syncthreads();
      if (owns) {
        for (int cc = len - 1; cc >= 0; --cc) {
          const T t = r1[cc] * r2[cc];
          acc += t;
        }
      }
    }
    if (c < len) {
      const T* const sx = FIRST ? s0 : s2;
#pragma unroll 4
      for (int r = half; r < nvalid; r += 2) x[sbase[r] + seg0 + c] = sx[r * P + c];
    }
    __syncthreads();
  }
  return acc;
}

template <class T>
__global__ __launch_bounds__(kMgLineGroup) void neptune_mg_line_contig(MgBox B, T* __restrict__ q, const T* __restrict__ b,
                                                                       const T* __restrict__ lo, const T* __restrict__ inv,
                                                                       const T* __restrict__ up, T* __restrict__ x) {
  (void)mg_line_contig_body<T, kMgLinePlain>(B, q, b, lo, inv, up, x);
}
// the apply-free stage on the contiguous axis: LDS as the plain form's
template <class T>
__global__ __launch_bounds__(kMgLineGroup) void neptune_mg_line_contig_first(MgBox B, const T* __restrict__ b, const T* __restrict__ lo,
                                                                             const T* __restrict__ inv, const T* __restrict__ up,
                                                                             T* __restrict__ x) {
  (void)mg_line_contig_body<T, kMgLineFirst>(B, (T*)nullptr, b, lo, inv, up, x);
}
// the stage with b . x_new on the contiguous axis: the workgroup is one wave, so its partial is that wave's sum on the
// shuffle tree of monitor_block_sum (whose sum over one wave this is, bit for bit) and needs no LDS word
template <class T>
__global__ __launch_bounds__(kMgLineGroup) void neptune_mg_line_contig_dot(MgBox B, T* __restrict__ q, const T* __restrict__ b,
                                                                           const T* __restrict__ lo, const T* __restrict__ inv,
                                                                           const T* __restrict__ up, T* __restrict__ x,
                                                                           T* __restrict__ partials) {
  static_assert(kMgLineGroup == kWave, "one wave per workgroup");
  T v = mg_line_contig_body<T, kMgLineDot>(B, q, b, lo, inv, up, x);
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  if (threadIdx.x == 0) {
    T r = 0;
    r += v;
    partials[linear_block()] = r;
  }
}

}  // namespace neptune_hip
