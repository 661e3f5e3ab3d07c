// The differentiable ghost refresh of the sharded path and its backward (spec in include/e3gnn.h): a row copy and a row sum
// over [n, D] with a leading dimension, fp32 or fp64.  Both are HBM-bound passes: one wave per row, lanes over 16-byte
// column groups (float4 / double2) when every pointer and every row pitch allows them, the D % (16 / sizeof(T)) columns left
// over -- or the whole row otherwise -- one element per lane.  The row index is wave-uniform, so slot[i], red_ptr[i] and the
// red_k of a row are scalar loads.  No atomics: a row's sum is taken by one wave in the list's order, bit-equal run to run.
// The 16-byte groups and their sum are e3_rows.h, shared with e3_cell_images.hip.
#include "e3_rows.h"

#include <algorithm>

namespace e3 {

// out[i] = slot[i] < 0 ? h[i] : recv[slot[i]]  (a slot >= n_recv reads nothing: the row is written as zero).
// DV = the 16-byte groups of a row (0: every column goes through the element loop)
template <typename T>
__global__ __launch_bounds__(256) void halo_refresh_kernel(const T* __restrict__ h, int64_t ld_h, const T* __restrict__ recv,
                                                           int64_t ld_r, int64_t n_recv, const int32_t* __restrict__ slot,
                                                           int64_t n, int DV, int D, T* __restrict__ out, int64_t ld_o) {
  using V = typename Vec16<T>::type;
  constexpr int VW = sizeof(V) / sizeof(T);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < n; i += nw) {
    const int s = slot[i];
    const T* src = s < 0 ? h + i * ld_h : (s < n_recv ? recv + (int64_t)s * ld_r : nullptr);
    T* dst = out + i * ld_o;
    for (int c = lane; c < DV; c += 64) {
      V v;
      vclear(v);
      if (src) v = reinterpret_cast<const V*>(src)[c];
      reinterpret_cast<V*>(dst)[c] = v;
    }
    for (int c = DV * VW + lane; c < D; c += 64) dst[c] = src ? src[c] : T(0);
  }
}

// out[i] = (slot[i] < 0 ? g[i] : 0) + sum_{q in [red_ptr[i], red_ptr[i+1])} back[red_k[q]], added in q order in T.
// The list bounds are clamped to [0, n_back] and a k outside [0, n_back) adds nothing: nothing is read out of bounds.
template <typename T>
__global__ __launch_bounds__(256) void halo_reduce_kernel(const T* __restrict__ g, int64_t ld_g, const T* __restrict__ back,
                                                          int64_t ld_b, int64_t n_back, const int32_t* __restrict__ slot,
                                                          const int32_t* __restrict__ red_ptr,
                                                          const int32_t* __restrict__ red_k, int64_t n, int DV, int D,
                                                          T* __restrict__ out, int64_t ld_o) {
  using V = typename Vec16<T>::type;
  constexpr int VW = sizeof(V) / sizeof(T);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < n; i += nw) {
    const bool owned = slot[i] < 0;
    int64_t b = 0, e = 0;
    if (n_back > 0) {
      b = red_ptr[i] < 0 ? 0 : red_ptr[i];
      e = red_ptr[i + 1] > n_back ? n_back : red_ptr[i + 1];
    }
    const T* grow = g + i * ld_g;
    T* dst = out + i * ld_o;
    for (int c = lane; c < DV; c += 64) {
      V acc;
      vclear(acc);
      if (owned) acc = reinterpret_cast<const V*>(grow)[c];
#pragma unroll 4
      for (int64_t q = b; q < e; ++q) {
        const int k = red_k[q];
        if (k >= 0 && k < n_back) vadd(acc, reinterpret_cast<const V*>(back + (int64_t)k * ld_b)[c]);
      }
      reinterpret_cast<V*>(dst)[c] = acc;
    }
    for (int c = DV * VW + lane; c < D; c += 64) {
      T acc = owned ? grow[c] : T(0);
#pragma unroll 4
      for (int64_t q = b; q < e; ++q) {
        const int k = red_k[q];
        if (k >= 0 && k < n_back) acc += back[(int64_t)k * ld_b + c];
      }
      dst[c] = acc;
    }
  }
}

static inline int row_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, 256 * 16)); }

template <typename T>
static int refresh_launch(const void* h, int64_t ld_h, const void* recv, int64_t ld_r, int64_t n_recv, const int32_t* slot,
                          int64_t n, int D, void* out, int64_t ld_o, hipStream_t s) {
  const int DV = groups16(D, sizeof(T), {h, recv, out}, {ld_h, ld_r, ld_o});
  hipLaunchKernelGGL(halo_refresh_kernel<T>, dim3(row_grid(n)), dim3(256), 0, s, (const T*)h, ld_h, (const T*)recv, ld_r,
                     n_recv, slot, n, DV, D, (T*)out, ld_o);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

template <typename T>
static int reduce_launch(const void* g, int64_t ld_g, const void* back, int64_t ld_b, int64_t n_back, const int32_t* slot,
                         const int32_t* red_ptr, const int32_t* red_k, int64_t n, int D, void* out, int64_t ld_o,
                         hipStream_t s) {
  const int DV = groups16(D, sizeof(T), {g, back, out}, {ld_g, ld_b, ld_o});
  hipLaunchKernelGGL(halo_reduce_kernel<T>, dim3(row_grid(n)), dim3(256), 0, s, (const T*)g, ld_g, (const T*)back, ld_b,
                     n_back, slot, red_ptr, red_k, n, DV, D, (T*)out, ld_o);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_halo_refresh(const void* h, int64_t ld_h, const void* recv, int64_t ld_recv, int64_t n_recv, const int32_t* slot,
                    int64_t n, int D, int dtype, void* out, int64_t ld_out, void* stream) {
  if (n < 0 || n_recv < 0 || D < 1 || ld_h < D || ld_recv < D || ld_out < D || (dtype != E3_F32 && dtype != E3_F64))
    return E3_ERR_INVALID_ARG;
  if (n == 0) return E3_OK;
  if (!h || !slot || !out || (n_recv > 0 && !recv)) return E3_ERR_INVALID_ARG;
  return dtype == E3_F32
             ? refresh_launch<float>(h, ld_h, recv, ld_recv, n_recv, slot, n, D, out, ld_out, (hipStream_t)stream)
             : refresh_launch<double>(h, ld_h, recv, ld_recv, n_recv, slot, n, D, out, ld_out, (hipStream_t)stream);
}

int e3_halo_reduce(const void* g, int64_t ld_g, const void* back, int64_t ld_back, int64_t n_back, const int32_t* slot,
                   const int32_t* red_ptr, const int32_t* red_k, int64_t n, int D, int dtype, void* out, int64_t ld_out,
                   void* stream) {
  if (n < 0 || n_back < 0 || D < 1 || ld_g < D || ld_back < D || ld_out < D || (dtype != E3_F32 && dtype != E3_F64))
    return E3_ERR_INVALID_ARG;
  if (n == 0) return E3_OK;
  if (!g || !slot || !out || (n_back > 0 && (!back || !red_ptr || !red_k))) return E3_ERR_INVALID_ARG;
  return dtype == E3_F32 ? reduce_launch<float>(g, ld_g, back, ld_back, n_back, slot, red_ptr, red_k, n, D, out, ld_out,
                                                (hipStream_t)stream)
                         : reduce_launch<double>(g, ld_g, back, ld_back, n_back, slot, red_ptr, red_k, n, D, out, ld_out,
                                                 (hipStream_t)stream);
}

}  // extern "C"
