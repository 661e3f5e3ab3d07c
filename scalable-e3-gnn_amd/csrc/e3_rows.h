// Row passes over [n, D] with a leading dimension (e3_halo_grad.hip, e3_cell_images.hip): the 16-byte column groups of a
// row and their element-wise sum.  A pass takes 16-byte accesses when every pointer and every row pitch allows them and
// goes element by element over the columns left over -- or over the whole row otherwise: same values either way.
#pragma once

#include "e3_common.h"

#include <initializer_list>

namespace e3 {

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

__device__ __forceinline__ void vclear(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vclear(double2& a) { a = make_double2(0.0, 0.0); }
__device__ __forceinline__ void vadd(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void vadd(double2& a, const double2 b) { a.x += b.x; a.y += b.y; }

// 16-byte groups of a row of D elements of `es` bytes, 0 unless every pointer and every pitch keeps them aligned
static inline int groups16(int D, int64_t es, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return 0;
  for (int64_t ld : lds)
    if ((ld * es) & 15) return 0;
  return (int)(D / (16 / es));
}

}  // namespace e3
