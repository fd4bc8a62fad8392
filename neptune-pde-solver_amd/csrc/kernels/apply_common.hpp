// apply_common.hpp -- shared device/host helpers for the NeptuneIR apply kernels (gfx950).
//
// Vocabulary (follows the reference's dialect, include/Dialect/NeptuneIR/*.td):
//   temp / field : dense row-major buffer of shape ub-lb for a logical box [lb,ub)
//   apply        : out<p> = body(p, access(k,off) = in_k<p+off>) for p in apply.bounds,
//                  out[q] = in_0[q] elsewhere (copy-through)
//   access       : read of input k at a compile-time offset from the current point
//   body         : the scalar region of the apply, evaluated in textual op order,
//                  strict IEEE (build with -ffp-contract=off)
//
// A *body functor* is what the lowering emits for one apply region (and what
// builtin_bodies.hpp hand-writes for the committed fixtures):
//
//   struct Body {
//     template <class A> __device__ T operator()(const A& a) const {
//       T c = a.template get<0, 0, 0, 0>();      // access %in0[0,0,0]
//       T w = a.template get<0, 0, 0, -1>();     // access %in0[0,0,-1]
//       long i = a.template idx<0>();            // region index argument #0
//       ...
//     }
//   };
//
// and a *footprint* describes, at compile time, which offsets the body touches so the
// march kernel knows what to keep in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace neptune_hip {

constexpr int kWave = 64;   // gfx950 wavefront
constexpr int kMaxRank = 3;
constexpr int kMaxInputs = 4;
constexpr int kNumXcd = 8;  // MI355X: 8 XCDs, workgroups dealt round-robin over them

// ---- compile-time loop: indices stay constants, arrays stay in VGPRs -----------------
template <class F, int... Is>
__host__ __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__host__ __device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// ---- footprint ------------------------------------------------------------------------
// HALO_INPUT : index of the (lowest) input read at non-zero offsets, or -1 if every access is
//              at offset 0 (a pointwise apply); HALO_MASK has one bit per such input.
// R0,R1,R2   : max |offset| of the halo inputs along the march (I), row (J) and contiguous (K)
//              axes *after* the rank mapping below.
// BOX        : true if some access has more than one non-zero offset component (27-point);
//              false for star stencils (5/7-point), which need no corner data.
template <int HALO_INPUT_, int R0_, int R1_, int R2_, bool BOX_, bool MARCH_OK_ = true,
          unsigned HALO_MASK_ = (HALO_INPUT_ >= 0 ? (1u << (HALO_INPUT_ < 0 ? 0 : HALO_INPUT_)) : 0u)>
struct Footprint {
  static constexpr int HALO_INPUT = HALO_INPUT_;  // lowest halo input (or -1); kept for readability
  // bit k set: input k is read at non-zero offsets and gets a register ring of its own.  Several
  // halo inputs (e.g. the h and q fields of a shallow-water residual) share the radii below.
  static constexpr unsigned HALO_MASK = HALO_MASK_;
  static constexpr int R0 = R0_, R1 = R1_, R2 = R2_;
  static constexpr bool BOX = BOX_;
  static constexpr bool MARCH_OK = MARCH_OK_;
};
constexpr int popcount_u(unsigned m) { int c = 0; for (; m; m &= m - 1) ++c; return c; }
// index of input `in` among the set bits of `mask` (its ring slot)
constexpr int halo_slot(unsigned mask, int in) { return popcount_u(mask & ((1u << in) - 1u)); }
// input index of ring slot `h`
constexpr int halo_input_of(unsigned mask, int h) {
  for (int k = 0; k < 32; ++k)
    if (mask & (1u << k)) { if (h == 0) return k; --h; }
  return -1;
}

// Value of a cell outside apply.bounds: input 0 at the same physical index (copy-through,
// DataflowLowering.cpp:283-287), unless the body functor supplies `T outside(T through) const` --
// the fused explicit time step does, because outside its rhs operator's bounds the rhs IS the
// copy-through of the state and the axpy still applies there.
template <class Body, class T, class = void>
struct OutsideOf {
  static __device__ __forceinline__ T apply(const Body&, T through) { return through; }
};
template <class Body, class T>
struct OutsideOf<Body, T, std::void_t<decltype(std::declval<const Body&>().outside(std::declval<T>()))>> {
  static __device__ __forceinline__ T apply(const Body& b, T through) { return b.outside(through); }
};

// ---- groups: sibling applies over shared inputs, one launch, one result per member --------------------
// A kernel asks ResultsOf<Body> how many results a body has (1 unless the body says NOUT).  A GroupBody carries the
// member bodies, one result pointer per member and, per member, the map from the member's input indices to the
// group's (the union of the members' operands): member bodies stay exactly what the lowering emits for a single
// apply, MappedAcc renumbers their accesses.  Member m's copy-through source is ITS input 0 -- group input
// THROUGH -- whose box equals the result's, so "input 0 at the same physical index" is that input's centre access.
template <class Body, class = void>
struct ResultsOf { static constexpr int value = 1; };
template <class Body>
struct ResultsOf<Body, std::void_t<decltype(Body::NOUT)>> { static constexpr int value = Body::NOUT; };

template <class A, class G>
struct MappedAcc {
  const A& a;
  template <int IN, int... O>
  __device__ __forceinline__ auto get() const { return a.template get<G::map(IN), O...>(); }
  template <int D>
  __device__ __forceinline__ int64_t idx() const { return a.template idx<D>(); }
};
template <class Body_, class FP_, int NIN_, int M0 = 0, int M1 = 1, int M2 = 2, int M3 = 3>
struct GroupMember {
  using Body = Body_;
  using FP = FP_;
  static constexpr int NIN = NIN_, THROUGH = M0;
  static constexpr int map(int k) { return k == 0 ? M0 : (k == 1 ? M1 : (k == 2 ? M2 : M3)); }
  Body body;
};
struct NoMember {};
template <class T, class G0, class G1, class G2 = NoMember, class G3 = NoMember>
struct GroupBody {
  static constexpr int NOUT = 2 + (std::is_same<G2, NoMember>::value ? 0 : 1) + (std::is_same<G3, NoMember>::value ? 0 : 1);
  static_assert(!std::is_same<G2, NoMember>::value || std::is_same<G3, NoMember>::value, "members are listed without gaps");
  G0 m0;
  G1 m1;
  G2 m2;
  G3 m3;
  T* out[4];
  template <int M> using Member = std::conditional_t<M == 0, G0, std::conditional_t<M == 1, G1, std::conditional_t<M == 2, G2, G3>>>;
  template <int M>
  __host__ __device__ __forceinline__ const Member<M>& member() const {
    if constexpr (M == 0) return m0;
    else if constexpr (M == 1) return m1;
    else if constexpr (M == 2) return m2;
    else return m3;
  }
  template <int M, class A>
  __device__ __forceinline__ T eval(const A& a) const { return member<M>().body(MappedAcc<A, Member<M>>{a}); }
  template <int M, class A>
  __device__ __forceinline__ T through(const A& a) const { return a.template get<Member<M>::THROUGH>(); }
  template <int M>
  __device__ __forceinline__ T outside(T thr) const { return OutsideOf<typename Member<M>::Body, T>::apply(member<M>().body, thr); }
};

// ---- monitored applies: the update norm S = sum (new - old)^2 out of the same launch ------------------
// A kernel asks IsMonitored<Body> whether the body is a MonitoredBody.  It then keeps one accumulator per lane, updated at
// the store site under the store's own predicates plus `inside` (cells outside apply.bounds, clamped or predicated-off
// cells and cells outside the launch region contribute nothing), reduces it over the workgroup after its last store and
// writes ONE partial at the workgroup's linear index; the host adds the partials in index order with a second kernel
// (apply_launch.hpp launch_apply_norm).  `old` is input 0 at the same physical index -- the copy-through source the store
// site holds anyway.  The wrapped body is evaluated exactly as on its own, so the result is the plain launch's, bit for bit.
struct MonitorPlan {     // host side of one monitored call: a counting pass sizes the partials, the launching pass fills them
  bool counting;         // true: launch nothing, add up the workgroups every launch of the call would have
  int64_t blocks;        // workgroups so far: where the next launch's partials start
  void* base;            // the partials buffer (launching pass)
};
// one term of S: two roundings (the difference, then the square), no FMA; a cell that does not count adds +0
template <class T>
__device__ __forceinline__ T monitor_term(bool counts, T fresh, T old) {
  const T d = fresh - old;
  const T q = d * d;
  return counts ? q : (T)0;
}
// The term policy of a monitored launch: what a counted cell adds, from the value the store site holds (`fresh`) and input 0
// at the same physical index (`old`).  MonitorDiffSq is the update norm's (fresh - old)^2 above; MonitorDot is one rounding
// of fresh * old -- with fresh = A(p) and old = p the launch returns p . A(p), the dot product a conjugate-gradient
// iteration needs.  A cell that does not count adds +0 through a select in both.
struct MonitorDiffSq {
  template <class T>
  static __device__ __forceinline__ T term(bool counts, T fresh, T old) { return monitor_term(counts, fresh, old); }
};
struct MonitorDot {
  template <class T>
  static __device__ __forceinline__ T term(bool counts, T fresh, T old) {
    const T q = fresh * old;
    return counts ? q : (T)0;
  }
};
template <class Body, class T, class Term_ = MonitorDiffSq>
struct MonitoredBody {
  static constexpr bool MONITORED = true;
  using Term = Term_;
  Body body;
  T* partials;           // this launch's partials, one per workgroup
  MonitorPlan* plan;     // host only
  template <class A>
  __device__ __forceinline__ T operator()(const A& a) const { return body(a); }
};
template <class Body, class = void>
struct IsMonitored { static constexpr bool value = false; };
template <class Body>
struct IsMonitored<Body, std::void_t<decltype(Body::MONITORED)>> { static constexpr bool value = true; };
template <class Body, class T, class Term>
struct OutsideOf<MonitoredBody<Body, T, Term>, T, void> {
  static __device__ __forceinline__ T apply(const MonitoredBody<Body, T, Term>& b, T through) { return OutsideOf<Body, T>::apply(b.body, through); }
};

// The workgroup's sum of `v`, valid in thread 0: wave shuffle tree, one slot per wave in `lds` (>= blockDim.x / 64 entries),
// the waves' sums added in wave order -- the same fixed tree as util_kernels.hpp's block_sum, which this header cannot
// include (that file holds a non-template kernel: one translation unit per library).  Every wave of the workgroup calls it.
template <class T>
__device__ __forceinline__ T monitor_block_sum(T v, T* lds) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = 0;
  if (threadIdx.x == 0) {
    const int nw = blockDim.x / kWave;
    for (int i = 0; i < nw; ++i) r += lds[i];
  }
  return r;
}
// The second kernel of a monitored call: ONE workgroup adds the n partials into *out.  Lane t adds a contiguous run of
// partials in index order, the 256 runs are added by the tree above in lane order: a fixed order, no atomics.
template <class T>
__global__ __launch_bounds__(256) void neptune_monitor_final(const T* __restrict__ partials, int64_t n, T* __restrict__ out) {
  __shared__ T lds[4];
  const int64_t per = (n + 255) / 256, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  T acc = 0;
  for (int64_t i = lo; i < hi; ++i) acc += partials[i];
  const T r = monitor_block_sum(acc, lds);
  if (threadIdx.x == 0) *out = r;
}

// Rank mapping onto the kernel's (I, J, K) axes.  K is always the contiguous last dim, I the
// slowest.  rank 3: (d0,d1,d2) -> (I,J,K); rank 2: (d0,d1) -> (I,K), J has extent 1;
// rank 1: (d0) -> (K), I and J have extent 1.
template <int RANK> struct AxisMap;
template <> struct AxisMap<3> { static constexpr int I = 0, J = 1, K = 2; };
template <> struct AxisMap<2> { static constexpr int I = 0, J = -1, K = 1; };
template <> struct AxisMap<1> { static constexpr int I = -1, J = -1, K = 0; };

template <int RANK, int AXIS_DIM, int... O>
struct PickOffset {
  static constexpr int value = [] {
    constexpr int offs[sizeof...(O) ? sizeof...(O) : 1] = {O...};
    return (AXIS_DIM >= 0 && AXIS_DIM < (int)sizeof...(O)) ? offs[AXIS_DIM < 0 ? 0 : AXIS_DIM] : 0;
  }();
};

// ---- deterministic test/bench field: exact on host and device ------------------------
// splitmix64 finaliser -> 24 (f32) or 53 (f64) mantissa bits -> [-1, 1)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ double hash_f64(int64_t index, uint64_t seed) {
  uint64_t h = mix64((uint64_t)index ^ mix64(seed));
  // 52 random bits -> [0,2) - 1 ; every step exact in binary64
  return (double)(h >> 12) * (1.0 / 2251799813685248.0) - 1.0;  // 2^-51
}
__host__ __device__ __forceinline__ float hash_f32(int64_t index, uint64_t seed) {
  uint64_t h = mix64((uint64_t)index ^ mix64(seed));
  return (float)(h >> 41) * (1.0f / 4194304.0f) - 1.0f;  // 23 bits * 2^-22
}

// ---- grids beyond 2^32 work-items --------------------------------------------------------------------
// HIP caps a grid dimension at 2^32 work-items (blocks x lanes), which a one-workgroup-per-256-cells launch
// over a 2048^3 field exceeds.  Such launches fold their workgroup count into (x, y).
constexpr uint32_t kMaxGridX = 1u << 22;  // x 256 lanes = 2^30 work-items along x
inline dim3 grid_for_blocks(int64_t blocks) {
  if (blocks <= (int64_t)kMaxGridX) return dim3((uint32_t)blocks);
  return dim3(kMaxGridX, (uint32_t)((blocks + kMaxGridX - 1) / kMaxGridX));
}
__device__ __forceinline__ int64_t linear_block() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// ---- XCD-aware workgroup id ------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Remap so that
// each XCD owns one contiguous run of virtual ids: neighbouring tiles (which share halo
// rows) then hit the same L2.  Bijective for any grid size; speed only, never correctness.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nb) {
  const uint32_t q = nb / kNumXcd, r = nb % kNumXcd;
  const uint32_t xcd = b % kNumXcd, pos = b / kNumXcd;
  return xcd < r ? xcd * (q + 1) + pos : r * (q + 1) + (xcd - r) * q + pos;
}

}  // namespace neptune_hip
