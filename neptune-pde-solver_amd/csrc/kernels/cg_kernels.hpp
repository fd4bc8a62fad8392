// cg_kernels.hpp -- the vector kernels of the device-resident conjugate-gradient solver (neptune_hip_cg_solve).
//
// One iteration is   q = A(p), pq = p . q        (a dot-monitored apply launch, apply_launch.hpp launch_apply_dot)
//                    x += alpha p, r -= alpha q, rr' = r . r      neptune_cg_update + neptune_cg_final
//                    p = r + beta p                               neptune_cg_direction
// alpha = rr / pq and beta = rr' / rr never leave the device: they live in a CgScalars block that the final kernel rotates,
// so every launch of an iteration has fixed arguments and a block of iterations can be replayed as a hipGraph.
// Arithmetic: everything in T, two roundings per update (the product, then the sum; build with -ffp-contract=off), sums on
// the fixed tree of the monitored applies -- per-lane accumulator, monitor_block_sum, one partial per workgroup at its linear
// index written by thread 0, one workgroup adds the partials in index order.  No atomics.  Templates only: the translation
// unit that holds the solver instantiates them.
#pragma once
#include "apply_common.hpp"

namespace neptune_hip {

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

// x = x + (alpha p), r = r - (alpha q) on all n cells of the flat buffers, and one partial of sum r * r (the freshly stored r)
// per workgroup.  16-byte vectors, exact grid, non-temporal stores (the shape of neptune_vec_update_v); the n % VK cells at
// the end go through lane 0 of workgroup 0.
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_update_v(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                           const T* __restrict__ q, T* __restrict__ x, T* __restrict__ r,
                                                           T* __restrict__ partials) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  __shared__ T lds[4];
  const T alpha = cg_alpha(s);
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T acc = (T)0;
  if (i < nv) {
    const V pv = reinterpret_cast<const V*>(p)[i];
    const V qv = reinterpret_cast<const V*>(q)[i];
    const V xv = reinterpret_cast<const V*>(x)[i];
    const V rv = reinterpret_cast<const V*>(r)[i];
    V xn, rn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T ap = alpha * pv[e];
      const T aq = alpha * qv[e];
      xn[e] = xv[e] + ap;
      rn[e] = rv[e] - aq;
      const T t = rn[e] * rn[e];
      acc += t;
    }
    __builtin_nontemporal_store(xn, reinterpret_cast<V*>(x) + i);
    __builtin_nontemporal_store(rn, reinterpret_cast<V*>(r) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T ap = alpha * p[j];
      const T aq = alpha * q[j];
      const T rn = r[j] - aq;
      x[j] = x[j] + ap;
      r[j] = rn;
      const T t = rn * rn;
      acc += t;
    }
  const T sum = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
// the same on operands that are not 16-byte aligned: grid-stride loop of scalar accesses (mirrors neptune_vec_update)
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_update(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                         const T* __restrict__ q, T* __restrict__ x, T* __restrict__ r,
                                                         T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = cg_alpha(s);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  T acc = (T)0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T ap = alpha * p[i];
    const T aq = alpha * q[i];
    const T rn = r[i] - aq;
    x[i] = x[i] + ap;
    r[i] = rn;
    const T t = rn * rn;
    acc += t;
  }
  const T sum = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// p = r + (beta p) on all n cells, beta from the scalar block: the two forms of the update kernel
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_direction_v(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                              T* __restrict__ p) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  const T beta = s->beta;
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const V rv = reinterpret_cast<const V*>(r)[i];
    const V pv = reinterpret_cast<const V*>(p)[i];
    V pn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T bp = beta * pv[e];
      pn[e] = rv[e] + bp;
    }
    __builtin_nontemporal_store(pn, reinterpret_cast<V*>(p) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T bp = beta * p[j];
      p[j] = r[j] + bp;
    }
}
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_direction(int64_t n, const CgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                            T* __restrict__ p) {
  const T beta = s->beta;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T bp = beta * p[i];
    p[i] = r[i] + bp;
  }
}

// The set-up: r = b - q on Omega = apply.bounds x launch region and +0 elsewhere, p = r, one partial of sum r * r per workgroup.
// Rows-form addressing (as neptune_apply_rows / neptune_reduce_partial_box): a workgroup owns ONE 256-cell chunk of one row of
// the box, so the row decode is workgroup-uniform scalar work.  All five fields share the box; per-axis arrays in (I, J, K)
// order, absent axes extent 1.
struct CgBoxParams {
  int64_t n[3];            // the box's extents
  int64_t lo[3], hi[3];    // Omega, physical: [lo, hi) per axis (empty where hi <= lo)
};
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_init(CgBoxParams P, int64_t nchunk, const T* __restrict__ b, const T* __restrict__ q,
                                                       T* __restrict__ r, T* __restrict__ p, T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term = (T)0;
  if (blk < P.n[0] * P.n[1] * nchunk) {   // (else: the folded grid's last row of workgroups)
    const int64_t row = blk / nchunk, c = blk - row * nchunk;
    const int64_t i = row / P.n[1], j = row - i * P.n[1];
    const int64_t k = c * 256 + threadIdx.x;
    if (k < P.n[2]) {
      const bool inside = i >= P.lo[0] && i < P.hi[0] && j >= P.lo[1] && j < P.hi[1] && k >= P.lo[2] && k < P.hi[2];
      const int64_t o = row * P.n[2] + k;
      const T d = b[o] - q[o];
      const T v = inside ? d : (T)0;
      r[o] = v;
      p[o] = v;
      term = v * v;
    }
  }
  const T sum = monitor_block_sum(term, lds);
  if (threadIdx.x == 0) partials[blk] = sum;
}

// The root of a sum and the scalar bookkeeping, ONE workgroup: lane t adds a contiguous run of the n partials in index
// order, the 256 runs are added by monitor_block_sum (the tree of neptune_monitor_final).  Thread 0 then, with plain stores,
//   start = true   (after neptune_cg_init)    rr = sum, everything else 0: iteration 0 is next
//   start = false  (after neptune_cg_update)  rr_new = sum, beta = rr_new / rr (0 if this iteration found rr == 0 or pq == 0),
//                  trace[2 k] = pq_k and trace[2 k + 1] = rr_(k+1) when a trace is kept (k = iter < trace_iters), then the
//                  rotation rr <- rr_new and iter <- k + 1.
template <class T>
__global__ __launch_bounds__(256) void neptune_cg_final(const T* __restrict__ partials, int64_t n, CgScalars<T>* __restrict__ s,
                                                        T* __restrict__ trace, int64_t trace_iters, bool start) {
  __shared__ T lds[4];
  const int64_t per = (n + 255) / 256, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  T acc = (T)0;
  for (int64_t i = lo; i < hi; ++i) acc += partials[i];
  const T sum = monitor_block_sum(acc, lds);
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

}  // namespace neptune_hip
