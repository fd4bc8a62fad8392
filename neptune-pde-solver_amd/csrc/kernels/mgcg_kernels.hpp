// mgcg_kernels.hpp -- the kernels of multigrid-preconditioned conjugate gradients (neptune_hip_mgcg_solve): CG
// whose preconditioner z = M(r) is one symmetric V-cycle of multigrid_kernels.hpp on A z = r from z = 0.
//
//   neptune_mgcg_init        r = b - q, z = minv * r on Omega, +0 elsewhere; rr_0 = r . r            the set-up, rows form over the box
//   neptune_mgcg_update      x += alpha p, r -= alpha q, z = minv * r, rr' = r . r                   reads p, q, minv, x, r; writes x, r, z: 8 passes
//   neptune_mg_smooth_dot    the smoothing sweep of 3.14 and sum over Omega of b * x_new             the cycle's last sweep: yields r . z
//   neptune_mgcg_direction   p = z + beta p                                                          3 passes
//   neptune_mgcg_final       the root of one sum and the scalar bookkeeping, ONE workgroup, four stages
//
// z is a field here (the cycle smooths it), and the update kernel stores the cycle's FIRST pre-sweep with it: from z = 0 and
// A(0) = 0 that sweep is z = 0 + minv * (r - 0) = minv * r, one rounding.  The cycle's LAST post-sweep is the kernel that holds
// b = r in a register when it stores the final z: it adds t = b * x_new to a workgroup sum, so r . z costs no pass.
//
// The frame is the one of krylov_kernels.hpp (flat_cells, the scalar block -- PcgScalars as it is --, block_partial_sums,
// final_partial_sums) and of multigrid_kernels.hpp (mg_row, mg_at).  Arithmetic: everything in T, every intermediate a named
// temporary, one rounding per operation (build with -ffp-contract=off); sums on the fixed tree of the monitored applies; no
// atomics.  Templates only: the translation unit that holds the solver instantiates them.
#pragma once
#include "krylov_kernels.hpp"
#include "multigrid_kernels.hpp"

namespace neptune_hip {

// The set-up: r = b - q on Omega and +0 elsewhere, z = minv * r on Omega and +0 elsewhere through the same select, one partial
// of sum r * r per workgroup of the (possibly folded) grid.  WITH_Z = false (level 0 smooths with line stages):
// r only -- minv and z are not touched and may be null
template <class T, bool WITH_Z = true>
__global__ __launch_bounds__(256) void neptune_mgcg_init(CgBoxParams P, int64_t nchunk, const T* __restrict__ b, const T* __restrict__ q,
                                                         const T* __restrict__ minv, T* __restrict__ r, T* __restrict__ z,
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
    if constexpr (WITH_Z) {
      const T zd = minv[o] * d;
      const T w = inside ? zd : (T)0;
      z[o] = w;
    }
    term = v * v;
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// x = x + (alpha p), r = r - (alpha q), z = minv * r (the freshly stored r) on all n cells, and one partial of sum r * r per
// workgroup.  alpha = rz / pq from the scalar block (pcg_alpha).  WITH_Z = false: x and r only -- reads p, q, x, r, writes x, r,
// 6 passes; minv and z are not touched and may be null
template <class T, bool VEC, bool WITH_Z = true>
__global__ __launch_bounds__(256) void neptune_mgcg_update(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                           const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ x,
                                                           T* __restrict__ r, T* __restrict__ z, T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = pcg_alpha(s);
  T acc = (T)0;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto pv = flat_load<W>(p, c), qv = flat_load<W>(q, c), xv = flat_load<W>(x, c), rv = flat_load<W>(r, c);
    flat_vec<T, W> mv, xn, rn, zn;
    if constexpr (WITH_Z) mv = flat_load<W>(minv, c);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T ap = alpha * pv[e];
      const T aq = alpha * qv[e];
      xn[e] = xv[e] + ap;
      rn[e] = rv[e] - aq;
      if constexpr (WITH_Z) zn[e] = mv[e] * rn[e];
      const T t = rn[e] * rn[e];
      acc += t;
    }
    flat_store<W>(x, c, xn);
    flat_store<W>(r, c, rn);
    if constexpr (WITH_Z) flat_store<W>(z, c, zn);
  });
  block_partial_sums({acc}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// The smoothing sweep of neptune_mg_smooth -- on Omega: d = b - q, w = minv * d, x = x + w -- and t = b * x_new, one rounding,
// into a workgroup sum: each lane owns one cell, so its accumulator is that one term (+0 for a lane without a cell).  One
// partial per workgroup of the (possibly folded) grid at its linear index.
template <class T>
__global__ __launch_bounds__(256) void neptune_mg_smooth_dot(MgBox B, int64_t nchunk, const T* __restrict__ q, const T* __restrict__ b,
                                                             const T* __restrict__ minv, T* __restrict__ x, T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term = (T)0;
  int64_t i, j, k0;
  if (mg_row(B, nchunk, blk, i, j, k0)) {
    const int64_t k = k0 + threadIdx.x;
    if (k < B.m[2]) {
      const int64_t o = mg_at(B, i, j, k);
      const T bv = b[o];
      const T d = bv - q[o];
      const T w = minv[o] * d;
      const T xn = x[o] + w;
      x[o] = xn;
      term = bv * xn;
    }
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// p = z + (beta p) on all n cells, beta from the scalar block
template <class T, bool VEC>
__global__ __launch_bounds__(256) void neptune_mgcg_direction(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ z,
                                                              T* __restrict__ p) {
  const T beta = s->beta;
  flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto zv = flat_load<W>(z, c), pv = flat_load<W>(p, c);
    flat_vec<T, W> pn;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const T bp = beta * pv[e];
      pn[e] = zv[e] + bp;
    }
    flat_store<W>(p, c, pn);
  });
}

// The root of one sum over partials[0 .. n) and the scalar bookkeeping, ONE workgroup.  Thread 0, with plain stores,
//   kMgcgStartRr  (after neptune_mgcg_init)          rr = the sum, everything else 0: iteration 0 is next
//   kMgcgStartRz  (after the set-up's cycle)         rz = the sum, *rz0 = the sum
//   kMgcgRr       (after neptune_mgcg_update)        rr_new = the sum
//   kMgcgRz       (after the iteration's cycle)      rz_new = the sum, beta = rz_new / rz (0 if this iteration found rz == 0 or
//                 pq == 0), trace[3 k .. 3 k + 2] = pq_k, rz_(k+1), rr_(k+1) when a trace is kept (k = iter < trace_iters), then the
//                 rotation rz <- rz_new, rr <- rr_new and iter <- k + 1.
enum : int { kMgcgStartRr = 0, kMgcgStartRz = 1, kMgcgRr = 2, kMgcgRz = 3 };
template <class T>
__global__ __launch_bounds__(256) void neptune_mgcg_final(const T* __restrict__ partials, int64_t n, PcgScalars<T>* __restrict__ s,
                                                          T* __restrict__ rz0, T* __restrict__ trace, int64_t trace_iters, int stage) {
  __shared__ T lds[4];
  T sum;
  final_partial_sums<1>(partials, n, lds, &sum);
  if (threadIdx.x != 0) return;
  if (stage == kMgcgStartRr) {
    s->rz = (T)0;
    s->rr = sum;
    s->pq = (T)0;
    s->rz_new = (T)0;
    s->rr_new = (T)0;
    s->beta = (T)0;
    s->iter = 0;
    *rz0 = (T)0;
  } else if (stage == kMgcgStartRz) {
    s->rz = sum;
    *rz0 = sum;
  } else if (stage == kMgcgRr) {
    s->rr_new = sum;
  } else {
    const T rz = s->rz, pq = s->pq, rr_new = s->rr_new;
    const int64_t k = s->iter;
    if (trace && k >= 0 && k < trace_iters) {
      trace[3 * k] = pq;
      trace[3 * k + 1] = sum;
      trace[3 * k + 2] = rr_new;
    }
    s->rz_new = sum;
    s->beta = (rz == (T)0 || pq == (T)0) ? (T)0 : sum / rz;
    s->rz = sum;
    s->rr = rr_new;
    s->iter = k + 1;
  }
}

}  // namespace neptune_hip
