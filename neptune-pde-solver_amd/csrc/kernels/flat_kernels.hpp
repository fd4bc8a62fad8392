// flat_kernels.hpp -- the frame of every kernel that streams flat buffers cell by cell: the Krylov vector updates of
// util_kernels.hpp and the solvers' kernels of krylov_kernels.hpp.
//
// Such a kernel exists in two forms, chosen by the host per launch (flat_grid):
//   VEC   every operand 16-byte aligned: one 16-byte group of VK = 16 / sizeof(T) cells per lane, exact grid of 256-lane
//         workgroups, non-temporal stores (the access pattern of the fastest copy kernel); the n % VK cells at the end go through
//         lane 0 of workgroup 0, one by one, AFTER that lane's group
//   else  a grid-stride loop of single cells on a capped grid
// Both forms run in workgroups of 256 lanes (flat_launch), and the frame counts on it.
// The frame owns the index arithmetic, the casts, the tail and the store policy; a kernel states its per-cell formula ONCE,
// in a generic lambda that flat_cells calls with a width tag W (VK or 1) and the first cell of the group:
//   flat_cells<T, VEC>(n, [&](auto w, int64_t c) {
//     constexpr int W = decltype(w)::value;
//     const auto xv = flat_load<W>(x, c);              // W cells from c on, as an ext_vector_type(W) value
//     flat_vec<T, W> yn;
//   #pragma unroll
//     for (int e = 0; e < W; ++e) { ... yn[e] = ...; acc += ...; }   // e ascending: the order of a lane's sum
//     flat_store<W>(y, c, yn);
//   });
// A kernel keeps its own __global__ signature with __restrict__ pointer parameters (in a struct they would not reach alias
// analysis) and writes every intermediate as a named T temporary (one rounding each; the build has -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

namespace neptune_hip {

template <int W> using flat_width = std::integral_constant<int, W>;
template <class T, int W> using flat_vec = T __attribute__((ext_vector_type(W)));

template <int W, class T>
__device__ __forceinline__ flat_vec<T, W> flat_load(const T* p, int64_t cell) {
  return *reinterpret_cast<const flat_vec<T, W>*>(p + cell);
}
// a plain store for a single cell, a non-temporal one for a 16-byte group
template <int W, class T>
__device__ __forceinline__ void flat_store(T* p, int64_t cell, flat_vec<T, W> v) {
  if constexpr (W == 1) p[cell] = v[0];
  else __builtin_nontemporal_store(v, reinterpret_cast<flat_vec<T, W>*>(p + cell));
}

// W cells that may span more than one 16-byte access (a group of 4 doubles next to 4 floats, mgcg_mixed_kernels.hpp): as
// 16-byte pieces, so that the operand needs 16-byte alignment only; W cells of at most 16 bytes: flat_load / flat_store
template <int W, class T>
__device__ __forceinline__ flat_vec<T, W> flat_load_wide(const T* p, int64_t cell) {
  constexpr int PK = 16 / (int)sizeof(T);
  if constexpr (W <= PK) {
    return flat_load<W>(p, cell);
  } else {
    static_assert(W % PK == 0, "whole 16-byte pieces");
    flat_vec<T, W> v;
#pragma unroll
    for (int h = 0; h < W / PK; ++h) {
      const auto piece = flat_load<PK>(p, cell + h * PK);
#pragma unroll
      for (int e = 0; e < PK; ++e) v[h * PK + e] = piece[e];
    }
    return v;
  }
}
template <int W, class T>
__device__ __forceinline__ void flat_store_wide(T* p, int64_t cell, flat_vec<T, W> v) {
  constexpr int PK = 16 / (int)sizeof(T);
  if constexpr (W <= PK) {
    flat_store<W>(p, cell, v);
  } else {
    static_assert(W % PK == 0, "whole 16-byte pieces");
#pragma unroll
    for (int h = 0; h < W / PK; ++h) {
      flat_vec<T, PK> piece;
#pragma unroll
      for (int e = 0; e < PK; ++e) piece[e] = v[h * PK + e];
      flat_store<PK>(p, cell + h * PK, piece);
    }
  }
}

// flat_cells for operands of more than one element size: the 16-byte form takes one group of VK cells per lane whatever the
// types (the kernel loads each operand with flat_load_wide), the tail and the grid-stride form are flat_cells'
template <int VK, bool VEC, class F>
__device__ __forceinline__ void flat_cells_group(int64_t n, F&& body) {
  if constexpr (VEC) {
    const int64_t nv = n / VK;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) body(flat_width<VK>{}, i * VK);
    if (i == 0)
      for (int64_t j = nv * VK; j < n; ++j) body(flat_width<1>{}, j);
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) body(flat_width<1>{}, i);
  }
}

template <class T, bool VEC, class F>
__device__ __forceinline__ void flat_cells(int64_t n, F&& body) {
  if constexpr (VEC) {
    constexpr int VK = 16 / (int)sizeof(T);
    const int64_t nv = n / VK;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) body(flat_width<VK>{}, i * VK);
    if (i == 0)
      for (int64_t j = nv * VK; j < n; ++j) body(flat_width<1>{}, j);
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) body(flat_width<1>{}, i);
  }
}

// ---- host side: which form a launch takes, and the launch itself
// exact for the 16-byte form (one group per lane; one workgroup when there is only a tail), capped at 256 * 32 workgroups for
// the grid-stride form
struct FlatGrid { bool vec; uint32_t blocks; };
inline FlatGrid flat_grid(int64_t n, size_t elem, std::initializer_list<const void*> ptrs) {
  bool aligned = true;
  for (const void* q : ptrs) aligned = aligned && (uintptr_t)q % 16 == 0;
  const int64_t nv = n / (int64_t)(16 / elem), vblocks = nv > 0 ? (nv + 255) / 256 : 1;
  if (aligned && vblocks <= 0x7fffffffLL) return {true, (uint32_t)vblocks};
  const int64_t want = (n + 255) / 256;
  return {false, (uint32_t)(want < 256 * 32 ? want : 256 * 32)};
}
// the grid of a flat_cells_group<vk> kernel: groups of `vk` cells whatever the operands' element sizes
inline FlatGrid flat_grid_group(int64_t n, int vk, std::initializer_list<const void*> ptrs) { return flat_grid(n, (size_t)(16 / vk), ptrs); }
// the two instantiations of one kernel and ONE argument list (converted to the kernel's parameter types): whichever form
// the grid asks for
template <class... P, class... A>
inline void flat_launch(const FlatGrid& g, hipStream_t stream, void (*vec)(P...), void (*cells)(P...), A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  hipLaunchKernelGGL(g.vec ? vec : cells, dim3(g.blocks), dim3(256), 0, stream, static_cast<P>(args)...);
}

}  // namespace neptune_hip
