// What the edge geometry kernels share: the device pieces of the three derivative kernels (e3_edge_geometry_bwd.hip) and the
// host pieces of their entries and of the forward's (e3_edge_ops.hip).  Every device helper is inlined into at least two
// kernels and is the text those kernels had: no floating-point expression is reordered here, and the reduction of the nine
// strain components -- which decides whether g_strain / h_strain are bitwise reproducible at S = 1 -- exists once.
#pragma once

#include "e3_common.h"

#include <type_traits>

namespace e3 {

constexpr float kS3 = 1.7320508075688772f, kS5 = 2.2360679774997896f;

// ---- device ---------------------------------------------------------------------------------------------------------------

// one edge of a row: r0 = x_src - x_dst (its minimum image in a box or cell), r = r0 + eps r0 when strained, d = |r|; behind
// the d > 0 guard, inv = 1 / d and u = r / d
struct EdgeVec {
  float r0x, r0y, r0z, rx, ry, rz, d, inv, x, y, z;
};
// r0, r and d of the edge pj -> pi; false for d = 0 (the forward uses u = 0 there, so the edge has no derivative: the backward
// and the Hessian skip it, the tangent writes zeros)
template <int PBC, bool STRAIN>
__device__ __forceinline__ bool edge_vec(const float4 pj, const float4 pi, const typename PbcArg<PBC>::type& box,
                                         const float eps[9], EdgeVec& ev) {
  edge_rel<PBC>(pj, pi, box, ev.rx, ev.ry, ev.rz);
  ev.r0x = ev.rx; ev.r0y = ev.ry; ev.r0z = ev.rz;
  if constexpr (STRAIN) apply_strain(eps, ev.rx, ev.ry, ev.rz);
  ev.d = sqrtf(ev.rx * ev.rx + ev.ry * ev.ry + ev.rz * ev.rz);
  return ev.d > 0.f;
}
// inv and u of an edge with d > 0
__device__ __forceinline__ void edge_unit(EdgeVec& ev) {
  ev.inv = 1.0f / ev.d;
  ev.x = ev.rx * ev.inv; ev.y = ev.ry * ev.inv; ev.z = ev.rz * ev.inv;
}

// one component of the cotangent of Y: the row's share gA[idx] / deg, and that of an edge, gY[idx] + the row's share (a NULL
// gradient is zeros).  By value, one component at a time: the kernels keep g and ga in registers from their first pass on
__device__ __forceinline__ float node_cotangent(const float* gA, const int64_t idx, const float invdeg) {
  return gA ? gA[idx] * invdeg : 0.f;
}
__device__ __forceinline__ float edge_cotangent(const float* gY, const int64_t idx, const float ga) {
  return (gY ? gY[idx] : 0.f) + ga;
}

__device__ __forceinline__ void atomic_add3(float* p, const float x, const float y, const float z) {
  atomicAdd(p + 0, x);
  atomicAdd(p + 1, y);
  atomicAdd(p + 2, z);
}
// sum of three values over the wave, in every lane (fixed butterfly)
__device__ __forceinline__ void wave_sum3(float& sx, float& sy, float& sz) {
  for (int o = 32; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o);
    sy += __shfl_xor(sy, o);
    sz += __shfl_xor(sz, o);
  }
}

// The nine strain components a lane has accumulated in G.  S > 1 (the rows of a structure are not contiguous): after every
// row, a butterfly per component, one 9-lane atomic into the row's structure dst [9] and G back to zero -- order of arrival,
// not bitwise reproducible.
__device__ __forceinline__ void strain_row_flush(float G[9], const int lane, float* dst) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
    if (lane == k) v = G[k];
    G[k] = 0.f;
  }
  if (lane < 9) atomicAdd(dst + lane, v);
}
// S = 1: once per workgroup of 4 waves, after all of its rows: a butterfly per component, the waves' sums through LDS and one
// 9-float partial per block in the order ((p0 + p1) + p2) + p3 -- on a fixed grid every sum has a fixed order, and
// strain_partial_sum_kernel adds the partials.  Called by every thread of the block.
__device__ __forceinline__ void strain_block_flush(float G[9], float* part_out) {
  __shared__ float part[4][9];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
    if (lane == 0) part[w][k] = G[k];
  }
  __syncthreads();
  if (threadIdx.x < 9)
    part_out[(int64_t)blockIdx.x * 9 + threadIdx.x] =
        ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// What the strained tangent and Hessian kernels take besides the arguments of the unstrained ones.  It is passed as a
// parameter pack that is empty in the unstrained kernels: a trailing parameter, even one of an empty type, would move their
// hidden arguments, and they are to stay the code they were before the strained forms existed.
struct StrainTangent {
  StrainArg st;
  const float* xi;   // [S,9] cotangent of g_strain | NULL
  float* hstrain;    // hvp: [S,9] | NULL
  float* hpart;      // hvp, S = 1: one 9-float partial per block
};
__device__ __forceinline__ const StrainTangent& only(const StrainTangent& sa) { return sa; }
// Xi of structure s into registers (zero for s = -1 or without a Xi: no read)
__device__ __forceinline__ void load_strain_cotangent(const float* xi, const int s, float x[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = (xi && s >= 0) ? xi[(int64_t)s * 9 + k] : 0.f;
}
// t <- (I + eps) t + Xi r
__device__ __forceinline__ void strain_tangent(const float e[9], const float xi[9], const float rx, const float ry,
                                               const float rz, float& tx, float& ty, float& tz) {
  apply_strain(e, tx, ty, tz);
  tx += xi[0] * rx + xi[1] * ry + xi[2] * rz;
  ty += xi[3] * rx + xi[4] * ry + xi[5] * rz;
  tz += xi[6] * rx + xi[7] * ry + xi[8] * rz;
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// The library's one open / orthorhombic dispatch of an entry that takes `box` NULL = open: f(mode, b) with mode a
// std::integral_constant of kOpen or kBox and b the kernel argument of the box (validated by the caller)
template <class F>
inline int dispatch_box(const float* box, F&& f) {
  const PbcBox b = make_box(box);
  return box ? f(std::integral_constant<int, kBox>{}, b) : f(std::integral_constant<int, kOpen>{}, b);
}

// what every derivative entry requires of (N, lmax), and a *_strained one of its strain [S,9] as well
inline bool geometry_args_valid(int64_t N, int lmax) { return N >= 0 && (lmax == 1 || lmax == 2); }
inline bool strained_args_valid(int64_t N, int lmax, const float* strain, int S) {
  return geometry_args_valid(N, lmax) && strain && S >= 1;
}
// S = 1 reduces its strain gradient through one partial per workgroup (strain_block_flush): with rows to reduce, the
// workspace must hold them
inline bool strain_workspace_valid(int S, int64_t N, const void* workspace, int64_t workspace_bytes) {
  return !(S == 1 && N > 0) || (workspace && workspace_bytes >= e3_edge_geometry_backward_strained_workspace_bytes(N));
}

}  // namespace e3
