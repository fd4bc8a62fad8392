// pcg_kernels.hpp -- the vector kernels of the Jacobi-preconditioned conjugate-gradient solver (neptune_hip_pcg_solve,
// DESIGN 3.12): the counterparts of cg_kernels.hpp with the diagonal preconditioner fused in.
//
// One iteration is   q = A(p), pq = p . q        (the dot-monitored apply launch of 3.11, unchanged)
//                    x += alpha p, r -= alpha q, rz' = r . (minv r), rr' = r . r      neptune_pcg_update + neptune_pcg_final
//                    p = (minv r) + beta p                                             neptune_pcg_direction
// z = minv r never exists as a field: both flat kernels that stream r form it in registers, one rounding, from the same two
// operands, so both see the same bits.  alpha = rz / pq and beta = rz' / rz live in a PcgScalars block.  Arithmetic and sums:
// as cg_kernels.hpp (everything in T, -ffp-contract=off, the fixed tree, no atomics); a kernel that forms two sums writes
// two partials per workgroup, the rz one at its linear index and the rr one `nblocks` further on.
#pragma once
#include "cg_kernels.hpp"

namespace neptune_hip {

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

// both workgroup sums of a kernel, one after the other through the same LDS words (monitor_block_sum ends on a barrier-free
// read of lds[0..3]: the barrier in between keeps the second sum's stores behind the first one's reads)
template <class T>
__device__ __forceinline__ void pcg_block_sums(T acc_rz, T acc_rr, T* lds, T* __restrict__ partials, int64_t blk, int64_t nblocks) {
  const T sum_rz = monitor_block_sum(acc_rz, lds);
  __syncthreads();
  const T sum_rr = monitor_block_sum(acc_rr, lds);
  if (threadIdx.x == 0) {
    partials[blk] = sum_rz;
    partials[nblocks + blk] = sum_rr;
  }
}

// x = x + (alpha p), r = r - (alpha q) on all n cells of the flat buffers, and per workgroup one partial of sum r * (minv * r)
// and one of sum r * r, both of the freshly stored r.  The shape of neptune_cg_update_v: 16-byte vectors, exact grid,
// non-temporal stores, the n % VK cells at the end through lane 0 of workgroup 0.
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_update_v(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                            const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ x,
                                                            T* __restrict__ r, T* __restrict__ partials) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  __shared__ T lds[4];
  const T alpha = pcg_alpha(s);
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T acc_rz = (T)0, acc_rr = (T)0;
  if (i < nv) {
    const V pv = reinterpret_cast<const V*>(p)[i];
    const V qv = reinterpret_cast<const V*>(q)[i];
    const V mv = reinterpret_cast<const V*>(minv)[i];
    const V xv = reinterpret_cast<const V*>(x)[i];
    const V rv = reinterpret_cast<const V*>(r)[i];
    V xn, rn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
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
      const T z = minv[j] * rn;
      const T tz = rn * z;
      const T tr = rn * rn;
      acc_rz += tz;
      acc_rr += tr;
    }
  pcg_block_sums(acc_rz, acc_rr, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}
// the same on operands that are not 16-byte aligned: grid-stride loop of scalar accesses (mirrors neptune_cg_update)
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_update(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                          const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ x,
                                                          T* __restrict__ r, T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = pcg_alpha(s);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  T acc_rz = (T)0, acc_rr = (T)0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T ap = alpha * p[i];
    const T aq = alpha * q[i];
    const T rn = r[i] - aq;
    x[i] = x[i] + ap;
    r[i] = rn;
    const T z = minv[i] * rn;
    const T tz = rn * z;
    const T tr = rn * rn;
    acc_rz += tz;
    acc_rr += tr;
  }
  pcg_block_sums(acc_rz, acc_rr, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// p = (minv r) + (beta p) on all n cells, beta from the scalar block: the two forms of the update kernel.  z = minv r is the
// product the update kernel summed: the same two operands, one rounding.
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_direction_v(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                               const T* __restrict__ minv, T* __restrict__ p) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  const T beta = s->beta;
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const V rv = reinterpret_cast<const V*>(r)[i];
    const V mv = reinterpret_cast<const V*>(minv)[i];
    const V pv = reinterpret_cast<const V*>(p)[i];
    V pn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T z = mv[e] * rv[e];
      const T bp = beta * pv[e];
      pn[e] = z + bp;
    }
    __builtin_nontemporal_store(pn, reinterpret_cast<V*>(p) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T z = minv[j] * r[j];
      const T bp = beta * p[j];
      p[j] = z + bp;
    }
}
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_direction(int64_t n, const PcgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                             const T* __restrict__ minv, T* __restrict__ p) {
  const T beta = s->beta;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T z = minv[i] * r[i];
    const T bp = beta * p[i];
    p[i] = z + bp;
  }
}

// The set-up: r = b - q on Omega and +0 elsewhere, p = minv r on Omega and +0 elsewhere through the same select, and per
// workgroup one partial of sum r * (minv * r) and one of sum r * r.  Addressing and arguments: neptune_cg_init; `nblocks` is
// the launch's workgroup count (the folded grid's: where the second partial array starts).
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_init(CgBoxParams P, int64_t nchunk, int64_t nblocks, const T* __restrict__ b,
                                                        const T* __restrict__ q, const T* __restrict__ minv, T* __restrict__ r,
                                                        T* __restrict__ p, T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t blk = linear_block();
  T term_rz = (T)0, term_rr = (T)0;
  if (blk < P.n[0] * P.n[1] * nchunk) {   // (else: the folded grid's last row of workgroups)
    const int64_t row = blk / nchunk, c = blk - row * nchunk;
    const int64_t i = row / P.n[1], j = row - i * P.n[1];
    const int64_t k = c * 256 + threadIdx.x;
    if (k < P.n[2]) {
      const bool inside = i >= P.lo[0] && i < P.hi[0] && j >= P.lo[1] && j < P.hi[1] && k >= P.lo[2] && k < P.hi[2];
      const int64_t o = row * P.n[2] + k;
      const T d = b[o] - q[o];
      const T zd = minv[o] * d;
      const T v = inside ? d : (T)0;
      const T z = inside ? zd : (T)0;
      r[o] = v;
      p[o] = z;
      term_rz = v * z;
      term_rr = v * v;
    }
  }
  pcg_block_sums(term_rz, term_rr, lds, partials, blk, nblocks);
}

// The roots of both sums and the scalar bookkeeping, ONE workgroup: as neptune_cg_final, on the two partial arrays
// partials[0 .. n) (rz) and partials[n .. 2 n) (rr), each added in index order on the same tree.  Thread 0 then, with plain stores,
//   start = true   (after neptune_pcg_init)    rz and rr = the sums, everything else 0: iteration 0 is next
//   start = false  (after neptune_pcg_update)  rz_new and rr_new = the sums, beta = rz_new / rz (0 if this iteration found
//                  rz == 0 or pq == 0), trace[3 k .. 3 k + 2] = pq_k, rz_(k+1), rr_(k+1) when a trace is kept
//                  (k = iter < trace_iters), then the rotation rz <- rz_new, rr <- rr_new and iter <- k + 1.
template <class T>
__global__ __launch_bounds__(256) void neptune_pcg_final(const T* __restrict__ partials, int64_t n, PcgScalars<T>* __restrict__ s,
                                                         T* __restrict__ trace, int64_t trace_iters, bool start) {
  __shared__ T lds[4];
  const int64_t per = (n + 255) / 256, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  T acc_rz = (T)0, acc_rr = (T)0;
  for (int64_t i = lo; i < hi; ++i) {
    acc_rz += partials[i];
    acc_rr += partials[n + i];
  }
  const T sum_rz = monitor_block_sum(acc_rz, lds);
  __syncthreads();
  const T sum_rr = monitor_block_sum(acc_rr, lds);
  if (threadIdx.x != 0) return;
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

}  // namespace neptune_hip
