// mgcg_mixed_kernels.hpp -- the seam between the two precisions of mixed-precision multigrid-preconditioned conjugate
// gradients (neptune_hip_mgcg_solve_mixed): x, b, r, p, q and every CG scalar in D = f64, the whole V-cycle of the
// preconditioner in S = f32 on a narrowed copy of the residual.
//
//   neptune_mgcg_init_mixed        r = b - q in D, r32 = narrow(r), z32 = minv * r32 in S on Omega, +0 elsewhere; rr_0 = r . r in D
//   neptune_mgcg_update_mixed      x += alpha p, r -= alpha q in D, r32 = narrow(r), z32 = minv * r32 in S, rr' = r . r in D
//                                  reads p, q, x, r (D) and minv (S); writes x, r (D) and r32, z32 (S): 6 D passes + 3 S passes
//   neptune_mg_smooth_dot_wide     the S sweep of neptune_mg_smooth and sum over Omega of (D)b * (D)x_new, exact per term, in D
//   neptune_mgcg_direction_mixed   p = widen(z32) + beta p in D: 2 D passes + 1 S pass; FIRST: p = widen(z32), the set-up's copy
//   neptune_mgcg_final<D>          (mgcg_kernels.hpp) the root of one sum and the scalar bookkeeping, as it is
//
// narrow is the cast (S)v: one rounding to nearest even, a finite value beyond S's range becomes +-inf, a result in S's
// subnormal range is kept (the build has no flush flag), -0 and NaN pass through.  widen is the cast (D)v: exact.
//
// The flat kernels work on groups of 4 cells per lane (flat_cells_group<4>): two 16-byte accesses per D operand, one per S
// operand, so that every access of the 16-byte form is 16 bytes wide.  The frame is the one of mgcg_kernels.hpp and
// krylov_kernels.hpp; arithmetic: operations on D values round in D, operations on S values round in S, every intermediate
// a named temporary, one rounding per operation (build with -ffp-contract=off); sums on the fixed tree of the monitored
// applies; no atomics.  Templates only: the translation unit that holds the solver instantiates them.
#pragma once
#include "mgcg_kernels.hpp"

namespace neptune_hip {

constexpr int kMixedGroup = 4;   // cells per lane of the 16-byte form: 32 bytes of D, 16 bytes of S

// The set-up: r = b - q on Omega and +0 elsewhere in D; r32 = narrow(r), z32 = minv * r32 on Omega and +0 elsewhere through
// the same select in S; one D partial of sum r * r per workgroup of the (possibly folded) grid
template <class D, class S>
__global__ __launch_bounds__(256) void neptune_mgcg_init_mixed(CgBoxParams P, int64_t nchunk, const D* __restrict__ b, const D* __restrict__ q,
                                                               const S* __restrict__ minv, D* __restrict__ r, S* __restrict__ r32,
                                                               S* __restrict__ z32, D* __restrict__ partials) {
  __shared__ D lds[4];
  const int64_t blk = linear_block();
  D term = (D)0;
  int64_t o;
  bool inside;
  if (box_cell(P, nchunk, blk, o, inside)) {
    const D d = b[o] - q[o];
    const D v = inside ? d : (D)0;
    r[o] = v;
    const S ds = (S)d;
    const S zd = minv[o] * ds;
    const S vs = inside ? ds : (S)0;
    const S ws = inside ? zd : (S)0;
    r32[o] = vs;
    z32[o] = ws;
    term = v * v;
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// x = x + (alpha p), r = r - (alpha q) in D, r32 = narrow(r) (the freshly stored r), z32 = minv * r32 in S on all n cells, and
// one D partial of sum r * r per workgroup.  alpha = rz / pq from the scalar block (pcg_alpha)
template <class D, class S, bool VEC>
__global__ __launch_bounds__(256) void neptune_mgcg_update_mixed(int64_t n, const PcgScalars<D>* __restrict__ s, const D* __restrict__ p,
                                                                 const D* __restrict__ q, const S* __restrict__ minv, D* __restrict__ x,
                                                                 D* __restrict__ r, S* __restrict__ r32, S* __restrict__ z32,
                                                                 D* __restrict__ partials) {
  __shared__ D lds[4];
  const D alpha = pcg_alpha(s);
  D acc = (D)0;
  flat_cells_group<kMixedGroup, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto pv = flat_load_wide<W>(p, c), qv = flat_load_wide<W>(q, c), xv = flat_load_wide<W>(x, c), rv = flat_load_wide<W>(r, c);
    const auto mv = flat_load<W>(minv, c);
    flat_vec<D, W> xn, rn;
    flat_vec<S, W> rs, zs;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const D ap = alpha * pv[e];
      const D aq = alpha * qv[e];
      xn[e] = xv[e] + ap;
      rn[e] = rv[e] - aq;
      rs[e] = (S)rn[e];
      zs[e] = mv[e] * rs[e];
      const D t = rn[e] * rn[e];
      acc += t;
    }
    flat_store_wide<W>(x, c, xn);
    flat_store_wide<W>(r, c, rn);
    flat_store<W>(r32, c, rs);
    flat_store<W>(z32, c, zs);
  });
  block_partial_sums({acc}, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// neptune_mg_smooth_dot<S> with a wide sum: the sweep's own arithmetic and stores are those of neptune_mg_smooth<S>; the
// term is t = (D)b * (D)x_new -- the product of two S values is exact in D --, the partials are D
template <class D, class S>
__global__ __launch_bounds__(256) void neptune_mg_smooth_dot_wide(MgBox B, int64_t nchunk, const S* __restrict__ q, const S* __restrict__ b,
                                                                  const S* __restrict__ minv, S* __restrict__ x, D* __restrict__ partials) {
  __shared__ D lds[4];
  const int64_t blk = linear_block();
  D term = (D)0;
  int64_t i, j, k0;
  if (mg_row(B, nchunk, blk, i, j, k0)) {
    const int64_t k = k0 + threadIdx.x;
    if (k < B.m[2]) {
      const int64_t o = mg_at(B, i, j, k);
      const S bv = b[o];
      const S d = bv - q[o];
      const S w = minv[o] * d;
      const S xn = x[o] + w;
      x[o] = xn;
      const D bw = (D)bv;
      const D xw = (D)xn;
      term = bw * xw;
    }
  }
  block_partial_sums({term}, lds, partials, blk, (int64_t)0);
}

// p = widen(z32) + (beta p) on all n cells, beta from the scalar block.  FIRST (the set-up): p = widen(z32); p is not read
// and `s` may be null
template <class D, class S, bool VEC, bool FIRST = false>
__global__ __launch_bounds__(256) void neptune_mgcg_direction_mixed(int64_t n, const PcgScalars<D>* __restrict__ s, const S* __restrict__ z32,
                                                                    D* __restrict__ p) {
  D beta = (D)0;
  if constexpr (!FIRST) beta = s->beta;
  flat_cells_group<kMixedGroup, VEC>(n, [&](auto w, int64_t c) {
    constexpr int W = decltype(w)::value;
    const auto zv = flat_load<W>(z32, c);
    flat_vec<D, W> pv, pn;
    if constexpr (!FIRST) pv = flat_load_wide<W>(p, c);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const D zw = (D)zv[e];
      if constexpr (FIRST) {
        pn[e] = zw;
      } else {
        const D bp = beta * pv[e];
        pn[e] = zw + bp;
      }
    }
    flat_store_wide<W>(p, c, pn);
  });
}

}  // namespace neptune_hip
