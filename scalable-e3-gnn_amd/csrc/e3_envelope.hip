// Smooth cutoff envelope and the weighted segment-sum pair (spec in include/e3gnn.h).
// The envelope kernels are elementwise over the edges.  The weighted sum and its backward are HBM-bound passes over
// [E, D]: one wave per CSR row (dst node), lanes over 16-byte column groups (4-byte ones when D, a stride or a pointer
// does not allow 16), four edges of the row in flight per column group, the row index -- and with it rowptr and w[e] --
// wave-uniform, so those are scalar loads.  Every sum has one fixed order: results are bit-equal from run to run.
#include "e3_common.h"

#include <algorithm>
#include <cmath>

namespace e3 {

// ---- envelope -------------------------------------------------------------------------------------------------------
// x = min(fl(d inv_rc), 1) (a NaN d stays NaN);  u = (1 - x)^3 sum_{k<p} C(k+2, 2) x^k by Horner from k = p - 1 down
__device__ __forceinline__ float envelope_x(const float d, const float inv_rc) {
  const float x = __fmul_rn(d, inv_rc);
  return x > 1.0f ? 1.0f : x;
}

__global__ __launch_bounds__(256) void cutoff_envelope_kernel(const float* __restrict__ edge_d, int64_t E, float r_c,
                                                              float inv_rc, int p, float* __restrict__ w) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < E; t += (int64_t)gridDim.x * blockDim.x) {
    const float d = edge_d[t];
    const float x = envelope_x(d, inv_rc);
    float s = (float)((p + 1) * p / 2);  // C(p + 1, 2), k = p - 1
    for (int k = p - 2; k >= 0; --k) s = fmaf(s, x, (float)((k + 2) * (k + 1) / 2));
    const float t1 = 1.0f - x;
    w[t] = d >= r_c ? 0.0f : (t1 * t1) * (t1 * s);
  }
}

// g_d = g_w du/dd,  du/dd = -(p (p+1) (p+2) / 2) x^(p-1) (1 - x)^2 / r_c
__global__ __launch_bounds__(256) void cutoff_envelope_bwd_kernel(const float* __restrict__ edge_d,
                                                                  const float* __restrict__ g_w, int64_t E, float r_c,
                                                                  float inv_rc, int p, float* __restrict__ g_d) {
  const float c = -(float)(p * (p + 1) * (p + 2) / 2);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < E; t += (int64_t)gridDim.x * blockDim.x) {
    const float d = edge_d[t];
    const float x = envelope_x(d, inv_rc);
    float xp = x;  // x^(p-1), p >= 2
    for (int k = 2; k < p; ++k) xp *= x;
    const float t1 = 1.0f - x;
    const float du = (c * xp) * (t1 * t1) * inv_rc;
    g_d[t] = d >= r_c ? 0.0f : g_w[t] * du;
  }
}

// backward of the backward, c = the cotangent of g_d:  cot_g_w = c du/dd,  cot_d = c g_w d2u/dd2,
// d2u/dd2 = -(p (p+1) (p+2) / 2) x^(p-2) (1 - x) ((p-1) (1 - x) - 2 x) / r_c^2   (x^0 = 1: p = 2 has no x factor)
__global__ __launch_bounds__(256) void cutoff_envelope_bwd2_kernel(const float* __restrict__ edge_d,
                                                                   const float* __restrict__ g_w,
                                                                   const float* __restrict__ cot, int64_t E, float r_c,
                                                                   float inv_rc, int p, float* __restrict__ cot_g_w,
                                                                   float* __restrict__ cot_d) {
  const float c = -(float)(p * (p + 1) * (p + 2) / 2);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < E; t += (int64_t)gridDim.x * blockDim.x) {
    const float d = edge_d[t];
    const float x = envelope_x(d, inv_rc);
    float xq = 1.0f;  // x^(p-2)
    for (int k = 2; k < p; ++k) xq *= x;
    const float t1 = 1.0f - x;
    const float du = (c * (xq * x)) * (t1 * t1) * inv_rc;
    const float d2u = (c * xq) * (t1 * ((float)(p - 1) * t1 - 2.0f * x)) * (inv_rc * inv_rc);
    const bool out = d >= r_c;
    const float cv = cot[t];
    if (cot_g_w) cot_g_w[t] = out ? 0.0f : cv * du;
    if (cot_d) cot_d[t] = out ? 0.0f : (cv * g_w[t]) * d2u;
  }
}

// ---- 4-byte / 16-byte column groups ---------------------------------------------------------------------------------
template <typename V> __device__ __forceinline__ V vzero();
template <> __device__ __forceinline__ float vzero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ void fma_to(float& a, const float w, const float v) { a = fmaf(w, v, a); }
__device__ __forceinline__ void fma_to(float4& a, const float w, const float4 v) {
  a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
}
__device__ __forceinline__ float scaled(const float w, const float g) { return __fmul_rn(w, g); }
__device__ __forceinline__ float4 scaled(const float w, const float4 g) {
  return make_float4(__fmul_rn(w, g.x), __fmul_rn(w, g.y), __fmul_rn(w, g.z), __fmul_rn(w, g.w));
}
__device__ __forceinline__ float dot_to(const float a, const float m, const float g) { return fmaf(m, g, a); }
__device__ __forceinline__ float dot_to(const float a, const float4 m, const float4 g) {
  return fmaf(m.w, g.w, fmaf(m.z, g.z, fmaf(m.y, g.y, fmaf(m.x, g.x, a))));
}

constexpr int kEdgesInFlight = 4;

// agg[i] = sum over CSR row i of w[e] msg[e]: edges in row order, one fmaf per element and edge.  V = float4 | float is the
// column group of a lane, G the groups a lane holds (64 G groups per pass over the row's edges); DV = D in units of V.
template <typename V, int G>
__global__ __launch_bounds__(256) void segment_sum_weighted_kernel(const float* __restrict__ msg, int64_t ld_msg,
                                                                   const float* __restrict__ w,
                                                                   const int32_t* __restrict__ rowptr, int64_t N, int DV,
                                                                   float* __restrict__ agg, int64_t ld_agg) {
  constexpr int VW = sizeof(V) / 4, K = kEdgesInFlight;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the row is wave-uniform: scalar loads below
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    for (int c0 = 0; c0 < DV; c0 += 64 * G) {
      V acc[G];
      bool act[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        acc[g] = vzero<V>();
        act[g] = c0 + 64 * g + lane < DV;
      }
      const float* col = msg + (int64_t)(c0 + lane) * VW;
      int q = b;
      for (; q + K <= e; q += K) {
        V v[K][G];
        float wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          wk[k] = w[q + k];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            v[k][g] = vzero<V>();
            if (act[g]) v[k][g] = *reinterpret_cast<const V*>(col + (int64_t)(q + k) * ld_msg + 64 * g * VW);
          }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int g = 0; g < G; ++g) fma_to(acc[g], wk[k], v[k][g]);
      }
      for (; q < e; ++q) {
        const float wq = w[q];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          V v = vzero<V>();
          if (act[g]) v = *reinterpret_cast<const V*>(col + (int64_t)q * ld_msg + 64 * g * VW);
          fma_to(acc[g], wq, v);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (act[g]) *reinterpret_cast<V*>(agg + i * ld_agg + (int64_t)(c0 + 64 * g + lane) * VW) = acc[g];
    }
  }
}

// sum of four per-lane values over the 64 lanes in 7 shuffles (a butterfly that halves the values kept at each of its first
// two steps): the sum of p[k] arrives in lane 16 k.  The lane order of every sum is fixed.
__device__ __forceinline__ float wave_sum4(const float p[4], const int lane) {
  const bool h32 = lane & 32, h16 = lane & 16;
  float k0 = h32 ? p[2] : p[0], k1 = h32 ? p[3] : p[1];
  k0 += __shfl_xor(h32 ? p[0] : p[2], 32);
  k1 += __shfl_xor(h32 ? p[1] : p[3], 32);
  float k = h16 ? k1 : k0;
  k += __shfl_xor(h16 ? k0 : k1, 16);
  for (int o = 8; o > 0; o >>= 1) k += __shfl_xor(k, o);
  return k;
}

// g_msg[e] = w[e] g_agg[dst(e)] (one rounding);  GW: g_w[e] = <msg[e], g_agg[dst(e)]>, per lane over its columns in column
// order, then wave_sum4.  ONE: the row's g_agg slice fits one pass (DV <= 64 G) and stays in registers across the edges.
template <typename V, int G, bool ONE, bool GW>
__global__ __launch_bounds__(256) void segment_sum_weighted_bwd_kernel(const float* __restrict__ gagg, int64_t ld_ga,
                                                                       const float* __restrict__ msg, int64_t ld_msg,
                                                                       const float* __restrict__ w,
                                                                       const int32_t* __restrict__ rowptr, int64_t N,
                                                                       int DV, float* __restrict__ gmsg, int64_t ld_gm,
                                                                       float* __restrict__ gw) {
  constexpr int VW = sizeof(V) / 4, K = kEdgesInFlight;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    if (b == e) continue;
    const float* grow = gagg + i * ld_ga;
    V gr[G];
    if constexpr (ONE) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        gr[g] = vzero<V>();
        if (64 * g + lane < DV) gr[g] = *reinterpret_cast<const V*>(grow + (int64_t)(64 * g + lane) * VW);
      }
    }
    for (int q = b; q < e; q += K) {
      const int nb = min(K, e - q);  // wave-uniform
      float wk[K], p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        wk[k] = k < nb ? w[q + k] : 0.f;
        p[k] = 0.f;
      }
      for (int c0 = 0; c0 < DV; c0 += 64 * G) {
        bool act[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          act[g] = c0 + 64 * g + lane < DV;
          if constexpr (!ONE) {
            gr[g] = vzero<V>();
            if (act[g]) gr[g] = *reinterpret_cast<const V*>(grow + (int64_t)(c0 + 64 * g + lane) * VW);
          }
        }
        const int64_t col = (int64_t)(c0 + lane) * VW;
        V m[K][G];
        if constexpr (GW) {
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int g = 0; g < G; ++g) {
              m[k][g] = vzero<V>();
              if (k < nb && act[g])
                m[k][g] = *reinterpret_cast<const V*>(msg + (int64_t)(q + k) * ld_msg + col + 64 * g * VW);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int g = 0; g < G; ++g) {
            if (k < nb && act[g])
              *reinterpret_cast<V*>(gmsg + (int64_t)(q + k) * ld_gm + col + 64 * g * VW) = scaled(wk[k], gr[g]);
            if constexpr (GW) p[k] = dot_to(p[k], m[k][g], gr[g]);
          }
        if constexpr (ONE) break;
      }
      if constexpr (GW) {
        const float s = wave_sum4(p, lane);
        if ((lane & 15) == 0 && (lane >> 4) < nb) gw[q + (lane >> 4)] = s;
      }
    }
  }
}

static inline int row_grid(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 256 * 16)); }
static inline int flat_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16)); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the envelope's arguments: p in [2, 16], r_c finite and > 0 with a finite fl(1 / r_c)
static inline bool envelope_args(float r_c, int p, float* inv_rc) {
  if (p < 2 || p > 16 || !(r_c > 0.0f) || !(r_c < 3.0e38f)) return false;
  *inv_rc = 1.0f / r_c;
  return *inv_rc < 3.0e38f;
}

template <typename V, bool GW>
static auto weighted_bwd_kernel(int DV) {
  return DV <= 64    ? segment_sum_weighted_bwd_kernel<V, 1, true, GW>
         : DV <= 128 ? segment_sum_weighted_bwd_kernel<V, 2, true, GW>
                     : segment_sum_weighted_bwd_kernel<V, 2, false, GW>;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_cutoff_envelope(const float* edge_d, int64_t E, float r_c, int p, float* w, void* stream) {
  float inv;
  if (E < 0 || !envelope_args(r_c, p, &inv)) return E3_ERR_INVALID_ARG;
  if (E == 0) return E3_OK;
  if (!edge_d || !w) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(cutoff_envelope_kernel, dim3(flat_grid(E)), dim3(256), 0, (hipStream_t)stream, edge_d, E, r_c, inv, p,
                     w);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_cutoff_envelope_backward(const float* edge_d, const float* g_w, int64_t E, float r_c, int p, float* g_d,
                                void* stream) {
  float inv;
  if (E < 0 || !envelope_args(r_c, p, &inv)) return E3_ERR_INVALID_ARG;
  if (E == 0) return E3_OK;
  if (!edge_d || !g_w || !g_d) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(cutoff_envelope_bwd_kernel, dim3(flat_grid(E)), dim3(256), 0, (hipStream_t)stream, edge_d, g_w, E, r_c,
                     inv, p, g_d);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_cutoff_envelope_backward2(const float* edge_d, const float* g_w, const float* c, int64_t E, float r_c, int p,
                                 float* cot_g_w, float* cot_d, void* stream) {
  float inv;
  if (E < 0 || !envelope_args(r_c, p, &inv) || !(inv * inv < 3.0e38f)) return E3_ERR_INVALID_ARG;
  if (E == 0 || (!cot_g_w && !cot_d)) return E3_OK;
  if (!edge_d || !c || (cot_d && !g_w)) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(cutoff_envelope_bwd2_kernel, dim3(flat_grid(E)), dim3(256), 0, (hipStream_t)stream, edge_d, g_w, c, E,
                     r_c, inv, p, cot_g_w, cot_d);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_segment_sum_weighted(const float* msg, int64_t ld_msg, const float* w, const int32_t* rowptr, int64_t N, int D,
                            float* agg, int64_t ld_agg, void* stream) {
  if (N < 0 || D <= 0 || ld_msg < D || ld_agg < D) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!msg || !w || !rowptr || !agg) return E3_ERR_INVALID_ARG;
  const bool vec = D % 4 == 0 && ld_msg % 4 == 0 && ld_agg % 4 == 0 && aligned16(msg) && aligned16(agg);
  const int DV = vec ? D / 4 : D;
  auto kern = vec ? (DV <= 64 ? segment_sum_weighted_kernel<float4, 1> : segment_sum_weighted_kernel<float4, 2>)
                  : (DV <= 64 ? segment_sum_weighted_kernel<float, 1> : segment_sum_weighted_kernel<float, 2>);
  hipLaunchKernelGGL(kern, dim3(row_grid(N)), dim3(256), 0, (hipStream_t)stream, msg, ld_msg, w, rowptr, N, DV, agg,
                     ld_agg);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_segment_sum_weighted_backward(const float* g_agg, int64_t ld_gagg, const float* msg, int64_t ld_msg, const float* w,
                                     const int32_t* rowptr, int64_t N, int D, float* g_msg, int64_t ld_gmsg, float* g_w,
                                     void* stream) {
  if (N < 0 || D <= 0 || ld_gagg < D || ld_gmsg < D || (g_w && ld_msg < D)) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!g_agg || !w || !rowptr || !g_msg || (g_w && !msg)) return E3_ERR_INVALID_ARG;
  const bool vec = D % 4 == 0 && ld_gagg % 4 == 0 && ld_gmsg % 4 == 0 && aligned16(g_agg) && aligned16(g_msg) &&
                   (!g_w || (ld_msg % 4 == 0 && aligned16(msg)));
  const int DV = vec ? D / 4 : D;
  auto kern = vec ? (g_w ? weighted_bwd_kernel<float4, true>(DV) : weighted_bwd_kernel<float4, false>(DV))
                  : (g_w ? weighted_bwd_kernel<float, true>(DV) : weighted_bwd_kernel<float, false>(DV));
  hipLaunchKernelGGL(kern, dim3(row_grid(N)), dim3(256), 0, (hipStream_t)stream, g_agg, ld_gagg, msg, ld_msg, w, rowptr, N,
                     DV, g_msg, ld_gmsg, g_w);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
