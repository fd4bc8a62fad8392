// krylov_kernels.hpp -- the vector kernels of the device-resident Krylov solvers: conjugate gradients (neptune_hip_cg_solve,
// DESIGN 3.11), its Jacobi-preconditioned form (neptune_hip_pcg_solve, 3.12) and BiCGStab (neptune_hip_bicgstab_solve, 3.13).
//
// CG        q = A(p), pq = p . q                      (a dot-monitored apply launch, apply_launch.hpp launch_apply_dot)
//           x += alpha p, r -= alpha q, rr' = r . r   neptune_cg_update + neptune_cg_final
//           p = r + beta p                            neptune_cg_direction
// PCG       the same with z = minv r:  rz' = r . z and rr' = r . r     neptune_pcg_update + neptune_pcg_final
//           p = z + beta p                                             neptune_pcg_direction
//           z never exists as a field: both kernels that stream r form it in registers, one rounding, from the same two
//           operands, so both see the same bits
// BiCGStab  v = A(p)                                  (a plain apply launch)
//           rv = rh . v                               neptune_bicg_rv + neptune_bicg_final(kBicgRv)
//           s = r - alpha v, in place in r            neptune_bicg_s
//           t = A(s), ts = t . s                      (the dot-monitored apply launch)
//           tt = t . t                                neptune_bicg_tt<.., false> + neptune_bicg_final(kBicgTt)
//             fallback: a plain launch, then ts and tt out of ONE pass: neptune_bicg_tt<.., true> + final(kBicgTsTt)
//           x += alpha p + omega s, r = s - omega t, rho' = rh . r, rr' = r . r
//                                                     neptune_bicg_update + neptune_bicg_final(kBicgUpdate)
//           p = r + beta (p - omega v)                neptune_bicg_direction
// The scalars (alpha, beta, omega and the sums they come from) never leave the device: they live in a scalar block that a
// one-workgroup kernel maintains with plain stores from thread 0, so every launch of an iteration has fixed arguments and a
// block of iterations can be replayed as a hipGraph.
//
// The frame, stated once.  Every kernel over all n cells of the flat buffers (update, direction, rv, s, tt) is a
// template <class T, bool VEC> on flat_cells (flat_kernels.hpp): its per-cell formula stands once, in one generic lambda,
// and the frame supplies the 16-byte form and the grid-stride form.  Arithmetic: everything in T, every intermediate a
// named temporary, one rounding per operation (build with -ffp-contract=off).  Sums on the fixed tree of the monitored
// applies: per-lane accumulator (cells in ascending order), monitor_block_sum, one partial per workgroup at its linear
// index written by thread 0 (block_partial_sums; a kernel with two sums puts the second one `nblocks` further on), one
// workgroup adds the partials in index order (final_partial_sums).  No atomics.  Templates only: the translation unit that
// holds the solvers instantiates them.
#pragma once
#include "apply_common.hpp"
#include "flat_kernels.hpp"

namespace neptune_hip {

// ---------------------------------------------------------------- what the kernels of all three solvers are built from
// One or two workgroup sums, one after the other through the same LDS words (monitor_block_sum ends on a barrier-free read
// of lds[0..3]: the barrier in between keeps the second sum's stores behind the first one's reads); thread 0 stores the
// first at partials[blk] and the second `nblocks` further on
template <class T, int NS>
__device__ __forceinline__ void block_partial_sums(const T (&acc)[NS], T* lds, T* __restrict__ partials, int64_t blk, int64_t nblocks) {
  static_assert(NS == 1 || NS == 2, "one sum or two");
  const T sum0 = monitor_block_sum(acc[0], lds);
  T sum1 = (T)0;
  if constexpr (NS == 2) {
    __syncthreads();
    sum1 = monitor_block_sum(acc[1], lds);
  }
  if (threadIdx.x == 0) {
    partials[blk] = sum0;
    if constexpr (NS == 2) partials[nblocks + blk] = sum1;
  }
}

// The roots of one or two sums in ONE workgroup: the first over partials[0 .. n), the second over partials[n .. 2 n); lane t
// adds a contiguous run of them in index order, the 256 runs are added by monitor_block_sum (the tree of
// neptune_monitor_final), with the barrier between two sums.  sum[] is thread 0's.  second = false (workgroup-uniform): the
// second sum has no partials and comes out as +0.
template <int NS, class T>
__device__ __forceinline__ void final_partial_sums(const T* __restrict__ partials, int64_t n, T* lds, T* sum, bool second = true) {
  static_assert(NS == 1 || NS == 2, "one sum or two");
  const int64_t per = (n + 255) / 256, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  T acc0 = (T)0, acc1 = (T)0;
  for (int64_t i = lo; i < hi; ++i) {
    acc0 += partials[i];
    if constexpr (NS == 2) {
      if (second) acc1 += partials[n + i];
    }
  }
  sum[0] = monitor_block_sum(acc0, lds);
  if constexpr (NS == 2) {
    __syncthreads();
    sum[1] = monitor_block_sum(acc1, lds);
  }
}

// The set-up kernels' addressing: rows form (as neptune_apply_rows / neptune_reduce_partial_box), a workgroup owns ONE 256-cell
// chunk of one row of the box, so the row decode is workgroup-uniform scalar work.  All of a solver's fields share the box;
// per-axis arrays in (I, J, K) order, absent axes extent 1.
struct CgBoxParams {
  int64_t n[3];            // the box's extents
  int64_t lo[3], hi[3];    // Omega, physical: [lo, hi) per axis (empty where hi <= lo)
};
// whether this lane of workgroup `blk` owns a cell (not: past the row's end, or the folded grid's last row of workgroups);
// -> o: the cell's flat index, inside: whether it lies in Omega
__device__ __forceinline__ bool box_cell(const CgBoxParams& P, int64_t nchunk, int64_t blk, int64_t& o, bool& inside) {
  if (blk >= P.n[0] * P.n[1] * nchunk) return false;
  const int64_t row = blk / nchunk, c = blk - row * nchunk;
  const int64_t i = row / P.n[1], j = row - i * P.n[1];
  const int64_t k = c * 256 + threadIdx.x;
  if (k >= P.n[2]) return false;
  inside = i >= P.lo[0] && i < P.hi[0] && j >= P.lo[1] && j < P.hi[1] && k >= P.lo[2] && k < P.hi[2];
  o = row * P.n[2] + k;
  return true;
}

// ---------------------------------------------------------------- conjugate gradients (3.11)
// The solver's device scalars.  rr: r . r of the current residual (what the host reads after a block of iterations);
// pq: p . A(p) of the iteration under way; rr_new: r . r after the update; beta: rr_new / rr as the final kernel formed it;
// iter: iterations completed.
template <class T>
struct CgScalars {
  T rr, pq, rr_new, beta;
  int64_t iter;
};

// alpha of the iteration under way: one division; an iteration that finds rr == 0 or pq == 0 uses alpha = beta = 0, so that
// nothing becomes NaN (the vectors stay as they are).  Every lane forms the same quotient from the same two operands.
template <class T>
__device__ __forceinline__ T cg_alpha(const CgScalars<T>* s) {
  const T rr = s->rr, pq = s->pq;
  return (rr == (T)0 || pq == (T)0) ? (T)0 : rr / pq;
}

// x = x + (alpha p), r = r - (alpha q) on all n cells, and one partial of sum r * r (the freshly stored r) per workgroup
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_cg_update(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                         const T* __restrict__ q, T* __restrict__ x, T* __restrict__ r,
                                                         T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = cg_alpha(s);
  T acc = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto pv = flat_load<W>(p, c), qv = flat_load<W>(q, c), xv = flat_load<W>(x, c), rv = flat_load<W>(r, c);
    flat_vec<T, W> xn, rn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T ap = alpha * pv[e];
      const T aq = alpha * qv[e];
      xn[e] = xv[e] + ap;
      rn[e] = rv[e] - aq;
      const T t = rn[e] * rn[e];
      acc += t;
    }
    flat_store<W>(x, c, xn);
    flat_store<W>(r, c, rn);
  });
  block_partial_sums({acc}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// p = r + (beta p) on all n cells, beta from the scalar block
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_cg_direction(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                            T* __restrict__ p) {
  const T beta = s->beta;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto rv = flat_load<W>(r, c), pv = flat_load<W>(p, c);
    flat_vec<T, W> pn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T bp = beta * pv[e];
      pn[e] = rv[e] + bp;
    }
    flat_store<W>(p, c, pn);
  });
}

// The set-up: r = b - q on Omega = apply.bounds x launch region and +0 elsewhere, p = r, one partial of sum r * r per workgroup
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_init(CgBoxParams P, int64_t nchunk, const T* __restrict__ b, const T* __restrict__ q,
                                                       T* __restrict__ r, T* __restrict__ p, T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term = (T)0;
  int64_t o;
  bool inside;
  if (box_cell(P, nchunk, blk, o, inside)) {
    const T d = b[o] - q[o];
    const T v = inside ? d : (T)0;
    r[o] = v;
    p[o] = v;
    term = v * v;
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// The root of a sum and the scalar bookkeeping, ONE workgroup.  Thread 0, with plain stores,
//   start = true   (after neptune_cg_init)    rr = sum, everything else 0: iteration 0 is next
//   start = false  (after neptune_cg_update)  rr_new = sum, beta = rr_new / rr (0 if this iteration found rr == 0 or pq == 0),
//                  trace[2 k] = pq_k and trace[2 k + 1] = rr_(k+1) when a trace is kept (k = iter < trace_iters), then the
//                  rotation rr <- rr_new and iter <- k + 1.
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_final(const T* __restrict__ partials, int64_t n, CgScalars<T>* __restrict__ s,
                                                        T* __restrict__ trace, int64_t trace_iters, bool start) {
  __shared__ T lds[4];
  T sum;
  final_partial_sums<1>(partials, n, lds, &sum);
  if (threadIdx.x != 0) return;
  if (start) {
    s->rr = sum;
    s->pq = (T)0;
    s->rr_new = (T)0;
    s->beta = (T)0;
    s->iter = 0;
    return;
  }
  const T rr = s->rr, pq = s->pq;
  const int64_t k = s->iter;
  if (trace && k >= 0 && k < trace_iters) {
    trace[2 * k] = pq;
    trace[2 * k + 1] = sum;
  }
  s->rr_new = sum;
  s->beta = (rr == (T)0 || pq == (T)0) ? (T)0 : sum / rr;
  s->rr = sum;
  s->iter = k + 1;
}

// ---------------------------------------------------------------- Jacobi-preconditioned conjugate gradients (3.12)
// The solver's device scalars.  rz: r . (minv r) of the current residual; rr: r . r of it (what the host reads after a block of
// iterations; after the set-up it reads the pair in one copy); pq: p . A(p) of the iteration under way; rz_new, rr_new: the two
// sums after the update; beta: rz_new / rz as the final kernel formed it; iter: iterations completed.  56 bytes for T = double.
template <class T>
struct PcgScalars {
  T rz, rr, pq, rz_new, rr_new, beta;
  int64_t iter;
};

// alpha of the iteration under way: one division; an iteration that finds rz == 0 or pq == 0 uses alpha = beta = 0
template <class T>
__device__ __forceinline__ T pcg_alpha(const PcgScalars<T>* s) {
  const T rz = s->rz, pq = s->pq;
  return (rz == (T)0 || pq == (T)0) ? (T)0 : rz / pq;
}

// x = x + (alpha p), r = r - (alpha q) on all n cells, and per workgroup one partial of sum r * (minv * r) and one of
// sum r * r, both of the freshly stored r
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_pcg_update(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                          const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ x,
                                                          T* __restrict__ r, T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = pcg_alpha(s);
  T acc_rz = (T)0, acc_rr = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto pv = flat_load<W>(p, c), qv = flat_load<W>(q, c), mv = flat_load<W>(minv, c), xv = flat_load<W>(x, c),
               rv = flat_load<W>(r, c);
    flat_vec<T, W> xn, rn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T ap = alpha * pv[e];
      const T aq = alpha * qv[e];
      xn[e] = xv[e] + ap;
      rn[e] = rv[e] - aq;
      const T z = mv[e] * rn[e];
      const T tz = rn[e] * z;
      const T tr = rn[e] * rn[e];
      acc_rz += tz;
      acc_rr += tr;
    }
    flat_store<W>(x, c, xn);
    flat_store<W>(r, c, rn);
  });
  block_partial_sums({acc_rz, acc_rr}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// p = (minv r) + (beta p) on all n cells, beta from the scalar block.  z = minv r is the product the update kernel summed:
// the same two operands, one rounding.
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_pcg_direction(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                             const T* __restrict__ minv, T* __restrict__ p) {
  const T beta = s->beta;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto rv = flat_load<W>(r, c), mv = flat_load<W>(minv, c), pv = flat_load<W>(p, c);
    flat_vec<T, W> pn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T z = mv[e] * rv[e];
      const T bp = beta * pv[e];
      pn[e] = z + bp;
    }
    flat_store<W>(p, c, pn);
  });
}

// The set-up: r = b - q on Omega and +0 elsewhere, p = minv r on Omega and +0 elsewhere through the same select, and per
// workgroup one partial of sum r * (minv * r) and one of sum r * r.  `nblocks` is the launch's workgroup count (the folded
// grid's: where the second partial array starts).
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_init(CgBoxParams P, int64_t nchunk, int64_t nblocks, const T* __restrict__ b,
                                                        const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ r,
                                                        T* __restrict__ p, T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term_rz = (T)0, term_rr = (T)0;
  int64_t o;
  bool inside;
  if (box_cell(P, nchunk, blk, o, inside)) {
    const T d = b[o] - q[o];
    const T zd = minv[o] * d;
    const T v = inside ? d : (T)0;
    const T z = inside ? zd : (T)0;
    r[o] = v;
    p[o] = z;
    term_rz = v * z;
    term_rr = v * v;
  }
  block_partial_sums({term_rz, term_rr}, lds, partials, blk, nblocks);
}

// The roots of both sums (rz over partials[0 .. n), rr over partials[n .. 2 n)) and the scalar bookkeeping, ONE workgroup.
// Thread 0, with plain stores,
//   start = true   (after neptune_pcg_init)    rz and rr = the sums, everything else 0: iteration 0 is next
//   start = false  (after neptune_pcg_update)  rz_new and rr_new = the sums, beta = rz_new / rz (0 if this iteration found
//                  rz == 0 or pq == 0), trace[3 k .. 3 k + 2] = pq_k, rz_(k+1), rr_(k+1) when a trace is kept
//                  (k = iter < trace_iters), then the rotation rz <- rz_new, rr <- rr_new and iter <- k + 1.
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_final(const T* __restrict__ partials, int64_t n, PcgScalars<T>* __restrict__ s,
                                                         T* __restrict__ trace, int64_t trace_iters, bool start) {
  __shared__ T lds[4];
  T sum[2];
  final_partial_sums<2>(partials, n, lds, sum);
  if (threadIdx.x != 0) return;
  const T sum_rz = sum[0], sum_rr = sum[1];
  if (start) {
    s->rz = sum_rz;
    s->pq = (T)0;
    s->rz_new = (T)0;
    s->beta = (T)0;
    s->rr = sum_rr;
    s->rr_new = (T)0;
    s->iter = 0;
    return;
  }
  const T rz = s->rz, pq = s->pq;
  const int64_t k = s->iter;
  if (trace && k >= 0 && k < trace_iters) {
    trace[3 * k] = pq;
    trace[3 * k + 1] = sum_rz;
    trace[3 * k + 2] = sum_rr;
  }
  s->rz_new = sum_rz;
  s->rr_new = sum_rr;
  s->beta = (rz == (T)0 || pq == (T)0) ? (T)0 : sum_rz / rz;
  s->rz = sum_rz;
  s->rr = sum_rr;
  s->iter = k + 1;
}

// ---------------------------------------------------------------- BiCGStab (3.13)
// The solver's device scalars.  rho: rh . r of the current residual; rv: rh . A(p), alpha: rho / rv, ts: A(s) . s, tt: A(s) . A(s),
// omega: ts / tt of the iteration under way; rho_new: rh . r after the update; rr: r . r of the current residual (what the host
// reads after a block of iterations); beta as the last bookkeeping kernel formed it; iter: iterations completed.  80 bytes
// for T = double.
template <class T>
struct BicgScalars {
  T rho, rv, alpha, ts, tt, omega, rho_new, rr, beta;
  int64_t iter;
};

// alpha of the iteration under way: one division; rho == 0 or rv == 0 gives alpha = 0, so that nothing becomes NaN.  Every lane
// (and the bookkeeping kernel, which stores it) forms the same quotient from the same two operands.
template <class T>
__device__ __forceinline__ T bicg_alpha(const BicgScalars<T>* s) {
  const T rho = s->rho, rv = s->rv;
  return (rho == (T)0 || rv == (T)0) ? (T)0 : rho / rv;
}

// one partial of sum a * b per workgroup, read-only: rv = rh . v
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_bicg_rv(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                       T* __restrict__ partials) {
  __shared__ T lds[4];
  T acc = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto av = flat_load<W>(a, c), bv = flat_load<W>(b, c);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T t = av[e] * bv[e];
      acc += t;
    }
  });
  block_partial_sums({acc}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// r = r - (alpha v) on all n cells, alpha formed from the scalar block: r then holds s
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_bicg_s(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ v,
                                                      T* __restrict__ r) {
  const T alpha = bicg_alpha(s);
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto vv = flat_load<W>(v, c), rv = flat_load<W>(r, c);
    flat_vec<T, W> sn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T av = alpha * vv[e];
      sn[e] = rv[e] - av;
    }
    flat_store<W>(r, c, sn);
  });
}

// read-only over t: one partial of sum t * t per workgroup (TWO = false; `sv` is not read), or -- the fallback, one pass over
// t and s -- one of sum t * s at the workgroup's index and one of sum t * t `gridDim.x` further on (TWO = true)
template <class T, bool VEC, bool TWO>
__global__ __launch_bounds__(256) void neptune_bicg_tt(int64_t n, const T* __restrict__ t, const T* __restrict__ sv,
                                                       T* __restrict__ partials) {
  __shared__ T lds[4];
  T acc_ts = (T)0, acc_tt = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto tv = flat_load<W>(t, c);
    auto ov = tv;
    if constexpr (TWO) ov = flat_load<W>(sv, c);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      if constexpr (TWO) {
        const T a = tv[e] * ov[e];
        acc_ts += a;
      }
      const T c2 = tv[e] * tv[e];
      acc_tt += c2;
    }
  });
  if constexpr (TWO) block_partial_sums({acc_ts, acc_tt}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
  else block_partial_sums({acc_tt}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// x = (x + (alpha p)) + (omega s), r = s - (omega t) on all n cells (s is what r holds on entry), and per workgroup one partial
// of sum rh * r and one of sum r * r, both of the freshly stored r.  alpha and omega: the scalar block's, as the bookkeeping
// kernel stored them.
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_bicg_update(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                           const T* __restrict__ t, const T* __restrict__ rh, T* __restrict__ x,
                                                           T* __restrict__ r, T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = s->alpha, omega = s->omega;
  T acc_rho = (T)0, acc_rr = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto sv = flat_load<W>(r, c), tv = flat_load<W>(t, c), pv = flat_load<W>(p, c), xv = flat_load<W>(x, c),
               hv = flat_load<W>(rh, c);
    flat_vec<T, W> xn, rn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T ap = alpha * pv[e];
      const T os = omega * sv[e];
      const T ot = omega * tv[e];
      const T xa = xv[e] + ap;
      xn[e] = xa + os;
      rn[e] = sv[e] - ot;
      const T th = hv[e] * rn[e];
      const T tr = rn[e] * rn[e];
      acc_rho += th;
      acc_rr += tr;
    }
    flat_store<W>(x, c, xn);
    flat_store<W>(r, c, rn);
  });
  block_partial_sums({acc_rho, acc_rr}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// p = r + (beta (p - (omega v))) on all n cells, beta and omega from the scalar block
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_bicg_direction(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                              const T* __restrict__ v, T* __restrict__ p) {
  const T beta = s->beta, omega = s->omega;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto rv = flat_load<W>(r, c), vv = flat_load<W>(v, c), pv = flat_load<W>(p, c);
    flat_vec<T, W> pn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T ov = omega * vv[e];
      const T d = pv[e] - ov;
      const T bd = beta * d;
      pn[e] = rv[e] + bd;
    }
    flat_store<W>(p, c, pn);
  });
}

// The set-up: r = b - q on Omega and +0 elsewhere, rh = r, p = r, one partial of sum r * r per workgroup (q is the field that
// holds A(x): the solver's v)
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_init(CgBoxParams P, int64_t nchunk, const T* __restrict__ b, const T* __restrict__ q,
                                                         T* __restrict__ r, T* __restrict__ rh, T* __restrict__ p,
                                                         T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term = (T)0;
  int64_t o;
  bool inside;
  if (box_cell(P, nchunk, blk, o, inside)) {
    const T d = b[o] - q[o];
    const T v = inside ? d : (T)0;
    r[o] = v;
    rh[o] = v;
    p[o] = v;
    term = v * v;
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// The roots of the sums and the scalar bookkeeping, ONE workgroup, after each reduction point: one sum over partials[0 .. n)
// and, where the stage has two, a second one over partials[n .. 2 n).  Thread 0, with plain stores,
//   kBicgStart   (after neptune_bicg_init)       rho = rr = the sum (ONE value: rh = r), everything else 0: iteration 0 is next
//   kBicgRv      (after neptune_bicg_rv)         rv = the sum, alpha = rho / rv (0 if rho == 0 or rv == 0)
//   kBicgTt      (after neptune_bicg_tt, one sum; ts is in the block already: the dot-monitored launch stored it)
//                                                tt = the sum, omega = ts / tt (0 if tt == 0)
//   kBicgTsTt    (after neptune_bicg_tt, two sums: the fallback)  ts and tt = the sums, omega likewise
//   kBicgUpdate  (after neptune_bicg_update)     rho_new and rr' = the sums, beta = (rho_new / rho) * (alpha / omega): two
//                divisions, then one product (0 if rho == 0, rv == 0 or omega == 0); trace[5 k .. 5 k + 4] = rv_k, ts_k, tt_k,
//                rho_(k+1), rr_(k+1) when a trace is kept (k = iter < trace_iters); then the rotation rho <- rho_new,
//                rr <- rr' and iter <- k + 1.
enum : int { kBicgStart = 0, kBicgRv = 1, kBicgTt = 2, kBicgTsTt = 3, kBicgUpdate = 4 };
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_final(const T* __restrict__ partials, int64_t n, BicgScalars<T>* __restrict__ s,
                                                          T* __restrict__ trace, int64_t trace_iters, int stage) {
  __shared__ T lds[4];
  const bool two = stage == kBicgTsTt || stage == kBicgUpdate;
  T sum[2];
  final_partial_sums<2>(partials, n, lds, sum, two);
  if (threadIdx.x != 0) return;
  const T sum0 = sum[0], sum1 = sum[1];
  if (stage == kBicgStart) {
    s->rho = sum0;
    s->rv = (T)0;
    s->alpha = (T)0;
    s->ts = (T)0;
    s->tt = (T)0;
    s->omega = (T)0;
    s->rho_new = (T)0;
    s->rr = sum0;
    s->beta = (T)0;
    s->iter = 0;
  } else if (stage == kBicgRv) {
    s->rv = sum0;
    s->alpha = bicg_alpha(s);
  } else if (stage == kBicgTt || stage == kBicgTsTt) {
    const T ts = two ? sum0 : s->ts, tt = two ? sum1 : sum0;
    s->ts = ts;
    s->tt = tt;
    s->omega = tt == (T)0 ? (T)0 : ts / tt;
  } else {
    const T rho = s->rho, rv = s->rv, alpha = s->alpha, omega = s->omega;
    const int64_t k = s->iter;
    if (trace && k >= 0 && k < trace_iters) {
      trace[5 * k] = rv;
      trace[5 * k + 1] = s->ts;
      trace[5 * k + 2] = s->tt;
      trace[5 * k + 3] = sum0;
      trace[5 * k + 4] = sum1;
    }
    T beta = (T)0;
    if (!(rho == (T)0 || rv == (T)0 || omega == (T)0)) {
      const T a = sum0 / rho;
      const T b = alpha / omega;
      beta = a * b;
    }
    s->rho_new = sum0;
    s->beta = beta;
    s->rho = sum0;
    s->rr = sum1;
    s->iter = k + 1;
  }
}

}  // namespace neptune_hip
