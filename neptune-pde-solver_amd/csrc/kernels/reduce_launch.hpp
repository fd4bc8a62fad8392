// reduce_launch.hpp -- host side of the reduce kernels: the launch plan of reduce(apply) (reduce_apply.hpp), its two
// launches, and the blocking read-back of a result.  The lowered runtime's fused reduce (run_apply_reduce_op,
// lowered_runtime.hpp) and the monitor's update norm (update_norm, neptune_hip_rt.hip) both launch through here, so the
// kernel choice and the grid are stated once; tests/reduce_cases.py restates them (MIRRORED).
#pragma once
#include "apply_launch.hpp"
#include "reduce_apply.hpp"

namespace neptune_hip {

struct ReduceApplyPlan {
  bool narrow;      // every coordinate fits the kernels' 32-bit indices; false: nothing may be launched
  bool vec;         // the vector kernel (16-byte loads), else the scalar one
  int64_t nchunk;   // row chunks per row of the reduced box
  int blocks;       // workgroups of the first pass = partials the root combines
};

// P.rlb / P.rub: the reduced box (not empty); ptrs: the inputs' base addresses; pointwise: every access of the body is at
// offset 0
template <class T, int NIN>
inline ReduceApplyPlan plan_reduce_apply(const DirectParams<T, NIN>& P, const void* const* ptrs, bool pointwise) {
  const int64_t eK = P.rub[2] - P.rlb[2];
  // pointwise body on 16-byte-aligned rows with all inputs in the result's box: the vector kernel
  constexpr int VK = 16 / (int)sizeof(T);
  bool vec = pointwise && eK % VK == 0 && P.rlb[2] % VK == 0 && P.n[2] % VK == 0;
  for (int k = 0; k < NIN; ++k) {
    vec = vec && ((uintptr_t)ptrs[k] % 16 == 0);
    for (int ax = 0; ax < 3; ++ax) vec = vec && P.sh[k][ax] == 0 && P.m[k][ax] == P.n[ax];
  }
  const int cells_per_chunk = 256 * (vec ? VK : 1), iter = vec ? kReduceApplyIter / 2 : kReduceApplyIter;
  const int64_t nchunk = (eK + cells_per_chunk - 1) / cells_per_chunk;
  const int64_t trips = ((P.rub[0] - P.rlb[0]) * (P.rub[1] - P.rlb[1]) * nchunk + iter - 1) / iter;
  const int blocks = (int)(trips < kReduceBlocks ? trips : kReduceBlocks);
  return {direct_params_narrow(P), vec, nchunk, blocks};
}

// the root of the tree over `blocks` partials of any first pass, into the device slot `result`
template <class T, class FOp>
inline void launch_reduce_root(const T* part, int blocks, T* result, hipStream_t st) {
  hipLaunchKernelGGL((neptune_reduce_final<T, FOp>), dim3(1), dim3(256), 0, st, part, blocks, result);
  NEPTUNE_HIP_CHECK(hipGetLastError());
}

// The first pass on POp into `part` (kReduceBlocks partials), then the root on FOp -- POp's combine, the identity map, the
// kind's finish -- into the device slot `result`.  POINTWISE: what the plan was given; a body that is not pointwise never
// instantiates the vector kernel.
template <class POp, class FOp, bool POINTWISE, class Body, class T, int RANK, int NIN>
inline void launch_reduce_apply(const ReduceApplyPlan& pl, const DirectParams<T, NIN>& P, const Body& body, T* part, T* result,
                                hipStream_t st) {
  const bool vec = POINTWISE && pl.vec;
  if constexpr (POINTWISE) {
    if (vec)
      hipLaunchKernelGGL((neptune_reduce_apply_vec<Body, T, RANK, NIN, POp>), dim3(pl.blocks), dim3(256), 0, st, P, body, pl.nchunk, part);
  }
  if (!vec)
    hipLaunchKernelGGL((neptune_reduce_apply<Body, T, RANK, NIN, POp>), dim3(pl.blocks), dim3(256), 0, st, P, body, pl.nchunk, part);
  launch_reduce_root<T, FOp>(part, pl.blocks, result, st);
}

// one device value of the element type, once the work queued on `st` is done; the widening keeps NaN, +-inf and -0
template <class T>
inline double read_back(const T* dev, hipStream_t st) {
  T h = 0;
  NEPTUNE_HIP_CHECK(hipMemcpyAsync(&h, dev, sizeof(T), hipMemcpyDeviceToHost, st));
  NEPTUNE_HIP_CHECK(hipStreamSynchronize(st));
  return (double)h;
}

}  // namespace neptune_hip
