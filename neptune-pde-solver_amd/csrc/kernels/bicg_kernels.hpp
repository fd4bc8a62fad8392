// bicg_kernels.hpp -- the vector kernels of the device-resident BiCGStab solver (neptune_hip_bicgstab_solve): the
// counterparts of cg_kernels.hpp / pcg_kernels.hpp for operators that are not symmetric.
//
// One iteration is   v = A(p)                                 (a plain apply launch)
//                    rv = rh . v                              neptune_bicg_rv + neptune_bicg_final(kBicgRv)
//                    s = r - alpha v, in place in r           neptune_bicg_s
//                    t = A(s), ts = t . s                     (the dot-monitored apply launch of 3.11, unchanged)
//                    tt = t . t                               neptune_bicg_tt<.., false> + neptune_bicg_final(kBicgTt)
//                      fallback: a plain launch, then ts and tt out of ONE pass: neptune_bicg_tt<.., true> + final(kBicgTsTt)
//                    x += alpha p + omega s, r = s - omega t, rho' = rh . r, rr' = r . r
//                                                             neptune_bicg_update + neptune_bicg_final(kBicgUpdate)
//                    p = r + beta (p - omega v)               neptune_bicg_direction
// alpha = rho / rv, omega = ts / tt and beta = (rho' / rho) (alpha / omega) live in a BicgScalars block that the one-workgroup
// kernel maintains with plain stores from thread 0, so every launch of an iteration has fixed arguments.  Arithmetic and sums:
// as cg_kernels.hpp (everything in T, one rounding per operation, -ffp-contract=off, the fixed tree, no atomics); a kernel
// that forms two sums writes two partials per workgroup, laid out as neptune_pcg_update_v's.
#pragma once
#include "pcg_kernels.hpp"

namespace neptune_hip {

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

// one partial of sum a * b per workgroup, read-only: rv = rh . v.  16-byte vectors, exact grid; the n % VK cells at the end go
// through lane 0 of workgroup 0.
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_rv_v(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                         T* __restrict__ partials) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  __shared__ T lds[4];
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T acc = (T)0;
  if (i < nv) {
    const V av = reinterpret_cast<const V*>(a)[i];
    const V bv = reinterpret_cast<const V*>(b)[i];
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T t = av[e] * bv[e];
      acc += t;
    }
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T t = a[j] * b[j];
      acc += t;
    }
  const T sum = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
// the same on operands that are not 16-byte aligned: grid-stride loop of scalar accesses
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_rv(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                       T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  T acc = (T)0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T t = a[i] * b[i];
    acc += t;
  }
  const T sum = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// r = r - (alpha v) on all n cells, alpha formed from the scalar block: r then holds s.  The two forms of neptune_cg_direction.
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_s_v(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ v,
                                                        T* __restrict__ r) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  const T alpha = bicg_alpha(s);
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const V vv = reinterpret_cast<const V*>(v)[i];
    const V rv = reinterpret_cast<const V*>(r)[i];
    V sn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T av = alpha * vv[e];
      sn[e] = rv[e] - av;
    }
    __builtin_nontemporal_store(sn, reinterpret_cast<V*>(r) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T av = alpha * v[j];
      r[j] = r[j] - av;
    }
}
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_s(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ v,
                                                      T* __restrict__ r) {
  const T alpha = bicg_alpha(s);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T av = alpha * v[i];
    r[i] = r[i] - av;
  }
}

// read-only over t: one partial of sum t * t per workgroup (TWO = false; `sv` is not read), or -- the fallback, one pass over
// t and s -- one of sum t * s at the workgroup's index and one of sum t * t `gridDim.x` further on (TWO = true)
template <class T, bool TWO>
__global__ __launch_bounds__(256) void neptune_bicg_tt_v(int64_t n, const T* __restrict__ t, const T* __restrict__ sv,
                                                         T* __restrict__ partials) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  __shared__ T lds[4];
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T acc_ts = (T)0, acc_tt = (T)0;
  if (i < nv) {
    const V tv = reinterpret_cast<const V*>(t)[i];
    V ov = tv;
    if (TWO) ov = reinterpret_cast<const V*>(sv)[i];
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      if (TWO) {
        const T a = tv[e] * ov[e];
        acc_ts += a;
      }
      const T c = tv[e] * tv[e];
      acc_tt += c;
    }
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      if (TWO) {
        const T a = t[j] * sv[j];
        acc_ts += a;
      }
      const T c = t[j] * t[j];
      acc_tt += c;
    }
  if (TWO) {
    pcg_block_sums(acc_ts, acc_tt, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
  } else {
    const T sum = monitor_block_sum(acc_tt, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
  }
}
template <class T, bool TWO>
__global__ __launch_bounds__(256) void neptune_bicg_tt(int64_t n, const T* __restrict__ t, const T* __restrict__ sv,
                                                       T* __restrict__ partials) {
  __shared__ T lds[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  T acc_ts = (T)0, acc_tt = (T)0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (TWO) {
      const T a = t[i] * sv[i];
      acc_ts += a;
    }
    const T c = t[i] * t[i];
    acc_tt += c;
  }
  if (TWO) {
    pcg_block_sums(acc_ts, acc_tt, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
  } else {
    const T sum = monitor_block_sum(acc_tt, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
  }
}

// x = (x + (alpha p)) + (omega s), r = s - (omega t) on all n cells (s is what r holds on entry), and per workgroup one partial
// of sum rh * r and one of sum r * r, both of the freshly stored r.  alpha and omega: the scalar block's, as the bookkeeping
// kernel stored them.  The shape of neptune_pcg_update_v.
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_update_v(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                             const T* __restrict__ t, const T* __restrict__ rh, T* __restrict__ x,
                                                             T* __restrict__ r, T* __restrict__ partials) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  __shared__ T lds[4];
  const T alpha = s->alpha, omega = s->omega;
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T acc_rho = (T)0, acc_rr = (T)0;
  if (i < nv) {
    const V pv = reinterpret_cast<const V*>(p)[i];
    const V tv = reinterpret_cast<const V*>(t)[i];
    const V hv = reinterpret_cast<const V*>(rh)[i];
    const V xv = reinterpret_cast<const V*>(x)[i];
    const V sv = reinterpret_cast<const V*>(r)[i];
    V xn, rn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
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
    __builtin_nontemporal_store(xn, reinterpret_cast<V*>(x) + i);
    __builtin_nontemporal_store(rn, reinterpret_cast<V*>(r) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T sj = r[j];
      const T ap = alpha * p[j];
      const T os = omega * sj;
      const T ot = omega * t[j];
      const T xa = x[j] + ap;
      const T rn = sj - ot;
      x[j] = xa + os;
      r[j] = rn;
      const T th = rh[j] * rn;
      const T tr = rn * rn;
      acc_rho += th;
      acc_rr += tr;
    }
  pcg_block_sums(acc_rho, acc_rr, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_update(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ p,
                                                           const T* __restrict__ t, const T* __restrict__ rh, T* __restrict__ x,
                                                           T* __restrict__ r, T* __restrict__ partials) {
  __shared__ T lds[4];
  const T alpha = s->alpha, omega = s->omega;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  T acc_rho = (T)0, acc_rr = (T)0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T si = r[i];
    const T ap = alpha * p[i];
    const T os = omega * si;
    const T ot = omega * t[i];
    const T xa = x[i] + ap;
    const T rn = si - ot;
    x[i] = xa + os;
    r[i] = rn;
    const T th = rh[i] * rn;
    const T tr = rn * rn;
    acc_rho += th;
    acc_rr += tr;
  }
  pcg_block_sums(acc_rho, acc_rr, lds, partials, (int64_t)blockIdx.x, (int64_t)gridDim.x);
}

// p = r + (beta (p - (omega v))) on all n cells, beta and omega from the scalar block: the two forms of the update kernel
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_direction_v(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                                const T* __restrict__ v, T* __restrict__ p) {
  constexpr int VK = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VK)));
  const T beta = s->beta, omega = s->omega;
  const int64_t nv = n / VK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const V rv = reinterpret_cast<const V*>(r)[i];
    const V vv = reinterpret_cast<const V*>(v)[i];
    const V pv = reinterpret_cast<const V*>(p)[i];
    V pn;
#pragma unroll
    for (int e = 0; e < VK; ++e) {
      const T ov = omega * vv[e];
      const T d = pv[e] - ov;
      const T bd = beta * d;
      pn[e] = rv[e] + bd;
    }
    __builtin_nontemporal_store(pn, reinterpret_cast<V*>(p) + i);
  }
  if (i == 0)
    for (int64_t j = nv * VK; j < n; ++j) {
      const T ov = omega * v[j];
      const T d = p[j] - ov;
      const T bd = beta * d;
      p[j] = r[j] + bd;
    }
}
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_direction(int64_t n, const BicgScalars<T>* __restrict__ s, const T* __restrict__ r,
                                                              const T* __restrict__ v, T* __restrict__ p) {
  const T beta = s->beta, omega = s->omega;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const T ov = omega * v[i];
    const T d = p[i] - ov;
    const T bd = beta * d;
    p[i] = r[i] + bd;
  }
}

// The set-up: r = b - q on Omega and +0 elsewhere, rh = r, p = r, one partial of sum r * r per workgroup.  Addressing and
// arguments: neptune_cg_init (q is the field that holds A(x): the solver's v).
template <class T>
__global__ __launch_bounds__(256) void neptune_bicg_init(CgBoxParams P, int64_t nchunk, const T* __restrict__ b, const T* __restrict__ q,
                                                         T* __restrict__ r, T* __restrict__ rh, T* __restrict__ p,
                                                         T* __restrict__ partials) {
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
      rh[o] = v;
      p[o] = v;
      term = v * v;
    }
  }
  const T sum = monitor_block_sum(term, lds);
  if (threadIdx.x == 0) partials[blk] = sum;
}

// The roots of the sums and the scalar bookkeeping, ONE workgroup, after each reduction point: as neptune_pcg_final, on the
// partial array partials[0 .. n) and, where the stage has two sums, partials[n .. 2 n), each added in index order on the same
// tree.  Thread 0 then, with plain stores,
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
  const int64_t per = (n + 255) / 256, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  T acc0 = (T)0, acc1 = (T)0;
  for (int64_t i = lo; i < hi; ++i) {
    acc0 += partials[i];
    if (two) acc1 += partials[n + i];
  }
  const T sum0 = monitor_block_sum(acc0, lds);
  __syncthreads();
  const T sum1 = monitor_block_sum(acc1, lds);
  if (threadIdx.x != 0) return;
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
