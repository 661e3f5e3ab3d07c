// Derivatives of the edge geometry (forward: e3_edge_ops.hip; spec in include/e3gnn.h): its backward in the positions and a
// strain -- what the force head (-dE/dpos, BASELINE.json configs[3]) and the stress need --, its tangent along a displacement
// field, and the Hessian-vector product of that backward, each in l_max 1 / 2 x open / box / cell x strained or not.  fp32,
// one wave per CSR row, HBM-bound streaming kernels.  The pieces the three kernels share are in e3_edge_geometry.h; what
// stays here per kernel is its arithmetic, in the expression order it has always had (the first-order kernel's g_u and the
// Hessian kernel's psi are the same quantity written in two orders, and round differently: they are not to be merged).
#include "e3_edge_geometry.h"

namespace e3 {

// Y = [1 | sqrt3 u | sqrt5 b(u)], u = r / |r|, r = x_src - x_dst; d = |r|; A_i = [1 | mean over the row of Y_e[1:]].
//   g_Yeff_e = gY_e + gA_dst[1:] / deg      (components >= 1)
//   g_u      = sqrt3 gY1 + sqrt5 (db/du)^T gY2
//   g_r      = (g_u - u (u . g_u)) / d + gd u          (0 for d = 0: the forward uses u = 0 there)
//   gpos[src] += g_r   (atomics),   gpos[dst] -= sum_e g_r   (wave reduction, one atomic per row and component)
// PBC: r is the minimum image of x_src - x_dst; the shift is piecewise constant, so dr/dx is that of the open box.
// STRAIN (r' = r + eps_s r, s = structure of the dst row): g' above is taken at r'; the position gradient is
// (I + eps_s)^T g', and G_s = dE/deps_s = sum over the structure's edges of g' (x) r (r unstrained) is reduced in the same
// pass.  S = 1: every lane sums its edges in registers over all of its wave's rows, the workgroup sums its waves through
// LDS and writes one 9-float partial per block to gpart (fixed grid: the order of every sum is fixed), and
// strain_partial_sum_kernel adds the partials.  S > 1: the rows of a structure are not contiguous, so each row is
// wave-reduced and added with one 9-lane atomic into G[s] (order of arrival: not bitwise reproducible).
template <int LMAX, int PBC, bool STRAIN>
__global__ __launch_bounds__(256) void edge_geometry_bwd_kernel(const float4* __restrict__ pos4,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ src, int64_t N,
                                                                const float* __restrict__ gY, const float* __restrict__ gd,
                                                                const float* __restrict__ gA, float* __restrict__ gpos,
                                                                const typename PbcArg<PBC>::type box, const StrainArg st,
                                                                float* __restrict__ gstrain, float* __restrict__ gpart) {
  constexpr int NY = (LMAX + 1) * (LMAX + 1);
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float G[9];
  if constexpr (STRAIN) {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = 0.f;
  }
  for (int64_t i = wave0; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    if (b == e) continue;
    const float4 pi = pos4[i];
    const float invdeg = 1.0f / (float)(e - b);
    float ga[NY];
#pragma unroll
    for (int k = 1; k < NY; ++k) ga[k] = node_cotangent(gA, i * NY + k, invdeg);
    int srow = 0;
    float eps[9];
    if constexpr (STRAIN) {
      srow = row_structure(st, i);
      load_strain(st, srow, eps);
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int q = b + lane; q < e; q += 64) {
      const int j = src[q];
      EdgeVec ev;
      if (!edge_vec<PBC, STRAIN>(pos4[j], pi, box, eps, ev)) continue;
      edge_unit(ev);
      const float inv = ev.inv, x = ev.x, y = ev.y, z = ev.z;
      float g[NY];
#pragma unroll
      for (int k = 1; k < NY; ++k) g[k] = edge_cotangent(gY, (int64_t)q * NY + k, ga[k]);
      float ux = kS3 * g[1], uy = kS3 * g[2], uz = kS3 * g[3];
      if constexpr (LMAX == 2) {
        // b0 = s3 x y, b1 = s3 y z, b2 = (2 z^2 - x^2 - y^2) / 2, b3 = s3 z x, b4 = (s3 / 2)(x^2 - y^2)
        const float c = kS5;
        ux += c * (kS3 * y * g[4] - x * g[6] + kS3 * z * g[7] + kS3 * x * g[8]);
        uy += c * (kS3 * x * g[4] + kS3 * z * g[5] - y * g[6] - kS3 * y * g[8]);
        uz += c * (kS3 * y * g[5] + 2.f * z * g[6] + kS3 * x * g[7]);
      }
      const float dot = x * ux + y * uy + z * uz;
      const float gdv = gd ? gd[q] : 0.f;
      float gx = (ux - x * dot) * inv + gdv * x, gy = (uy - y * dot) * inv + gdv * y,
            gz = (uz - z * dot) * inv + gdv * z;
      if constexpr (STRAIN) {
        if (srow >= 0) {
          G[0] += gx * ev.r0x; G[1] += gx * ev.r0y; G[2] += gx * ev.r0z;
          G[3] += gy * ev.r0x; G[4] += gy * ev.r0y; G[5] += gy * ev.r0z;
          G[6] += gz * ev.r0x; G[7] += gz * ev.r0y; G[8] += gz * ev.r0z;
        }
        const float tx = gx + (eps[0] * gx + eps[3] * gy + eps[6] * gz);
        const float ty = gy + (eps[1] * gx + eps[4] * gy + eps[7] * gz);
        const float tz = gz + (eps[2] * gx + eps[5] * gy + eps[8] * gz);
        gx = tx; gy = ty; gz = tz;
      }
      atomic_add3(gpos + (int64_t)j * 3, gx, gy, gz);
      sx += gx; sy += gy; sz += gz;
    }
    wave_sum3(sx, sy, sz);
    if (lane == 0) atomic_add3(gpos + i * 3, -sx, -sy, -sz);
    if constexpr (STRAIN)
      if (st.S > 1 && srow >= 0) strain_row_flush(G, lane, gstrain + (int64_t)srow * 9);
  }
  if constexpr (STRAIN)
    if (st.S == 1) strain_block_flush(G, gpart);
}

// G[k] = sum of the per-block partials gpart[p, k] of strain_block_flush (S = 1): one wave per component, lanes over
// the partials in a fixed order (16 loads in flight per lane before their adds), then a fixed butterfly
__global__ __launch_bounds__(576) void strain_partial_sum_kernel(const float* __restrict__ gpart, int nparts,
                                                                 float* __restrict__ gstrain) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  float acc = 0.f;
  int p = lane;
  for (; p + 15 * 64 < nparts; p += 16 * 64) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = gpart[(int64_t)(p + u * 64) * 9 + k];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += v[u];
  }
  for (; p < nparts; p += 64) acc += gpart[(int64_t)p * 9 + k];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) gstrain[k] = acc;
}

// Tangent of the edge geometry along a displacement field v [N,3] (include/e3gnn.h, e3_edge_geometry_jvp): the backward above
// is linear in (gY, gd, gA), so this is its backward w.r.t. those three.  t = v[src] - v[dst];  du = (t - u (u . t)) / d;
//   dY1 = sqrt3 du,  dY2 = sqrt5 (db/du) du  (b as above),  dd = u . t,  dA_i = (1 / deg_i) sum over the row of dY_e.
// One wave per row, lanes over its edges; dA: per-lane sums in edge order, then a fixed butterfly -- no atomics.
// STRAIN (e3_edge_geometry_jvp_strained): u and d are those of r' = (I + eps_s) r and the tangent of r' is
// t' = (I + eps_s) t + Xi_s r, Xi [S,9] the cotangent of g_strain (r unstrained); v or Xi may be NULL (zeros).  eps_s and Xi_s
// are read once per row with a wave-uniform structure id; a row outside [0, S) has eps = Xi = 0.
template <int LMAX, int PBC, bool STRAIN, class... SA>
__global__ __launch_bounds__(256) void edge_geometry_jvp_kernel(const float4* __restrict__ pos4,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ src, int64_t N,
                                                                const float* __restrict__ v, float* __restrict__ dY,
                                                                float* __restrict__ dd, float* __restrict__ dA,
                                                                const typename PbcArg<PBC>::type box, const SA... tail) {
  static_assert(sizeof...(SA) == (STRAIN ? 1 : 0), "the strained kernels take one StrainTangent, the others nothing");
  constexpr int NY = (LMAX + 1) * (LMAX + 1);
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    if (b == e) {
      if (dA && lane < NY) dA[i * NY + lane] = 0.f;
      continue;
    }
    const float4 pi = pos4[i];
    // v[i]; the strained kernels take a NULL v as zeros, the others load unconditionally (the test folds away)
    const float vix = (!STRAIN || v) ? v[i * 3 + 0] : 0.f, viy = (!STRAIN || v) ? v[i * 3 + 1] : 0.f,
                viz = (!STRAIN || v) ? v[i * 3 + 2] : 0.f;
    float eps[9], xi[9];
    if constexpr (STRAIN) {
      const StrainTangent& sa = only(tail...);
      const int srow = row_structure(sa.st, i);
      load_strain(sa.st, srow, eps);
      load_strain_cotangent(sa.xi, srow, xi);
    }
    float s[NY];
#pragma unroll
    for (int k = 0; k < NY; ++k) s[k] = 0.f;
    for (int q = b + lane; q < e; q += 64) {
      const int j = src[q];
      EdgeVec ev;
      const bool nonzero = edge_vec<PBC, STRAIN>(pos4[j], pi, box, eps, ev);
      float o[NY], ddv = 0.f;
#pragma unroll
      for (int k = 0; k < NY; ++k) o[k] = 0.f;
      if (nonzero) {
        edge_unit(ev);
        const float inv = ev.inv, x = ev.x, y = ev.y, z = ev.z;
        float tx = ((!STRAIN || v) ? v[(int64_t)j * 3 + 0] : 0.f) - vix;
        float ty = ((!STRAIN || v) ? v[(int64_t)j * 3 + 1] : 0.f) - viy;
        float tz = ((!STRAIN || v) ? v[(int64_t)j * 3 + 2] : 0.f) - viz;
        if constexpr (STRAIN) strain_tangent(eps, xi, ev.r0x, ev.r0y, ev.r0z, tx, ty, tz);
        ddv = x * tx + y * ty + z * tz;
        const float ux = (tx - x * ddv) * inv, uy = (ty - y * ddv) * inv, uz = (tz - z * ddv) * inv;
        o[1] = kS3 * ux; o[2] = kS3 * uy; o[3] = kS3 * uz;
        if constexpr (LMAX == 2) {
          o[4] = kS5 * kS3 * (y * ux + x * uy);
          o[5] = kS5 * kS3 * (z * uy + y * uz);
          o[6] = kS5 * (2.f * z * uz - x * ux - y * uy);
          o[7] = kS5 * kS3 * (x * uz + z * ux);
          o[8] = kS5 * kS3 * (x * ux - y * uy);
        }
      }
      if (dY) {
#pragma unroll
        for (int k = 0; k < NY; ++k) dY[(int64_t)q * NY + k] = o[k];
      }
      if (dd) dd[q] = ddv;
#pragma unroll
      for (int k = 1; k < NY; ++k) s[k] += o[k];
    }
    if (dA) {
      const float invdeg = 1.0f / (float)(e - b);
#pragma unroll
      for (int k = 1; k < NY; ++k)
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
      if (lane == 0) {
        dA[i * NY] = 0.f;
#pragma unroll
        for (int k = 1; k < NY; ++k) dA[i * NY + k] = s[k] * invdeg;
      }
    }
  }
}

// Backward of edge_geometry_bwd_kernel in the positions (include/e3gnn.h, e3_edge_geometry_hvp): hpos = d<v, gpos>/dpos.  Per
// edge gpos gets +-grad phi, phi(r) = <g, Y(r)> + gd |r| with g as above, so hpos gets +-(Hess phi) t, t = v[src] - v[dst].
// On the sphere <g, Y> = a1 . u + u^T Q u / 2 (a1 = sqrt3 g[1..3], Q the symmetric matrix of the l = 2 components of g), and
// psi = a1 + Q u is the (ux, uy, uz) of the kernel above.  With P = I - u u^T, du = P t / d, dd = u . t:
//   h = [ -(du (u . psi) + u (du . psi)) + P Q du ] / d  -  P psi dd / d^2  +  gd du
// Same shape as the first-order kernel: one wave per row, atomics into hpos[src], one wave reduction per row for hpos[dst].
// STRAIN (e3_edge_geometry_hvp_strained; M = I + eps_s, Xi the cotangent of g_strain, r unstrained): the formula above at
// r' = M r applied to t' = M t + Xi_s r gives w = (Hess phi)(r') t', and with g' = grad phi(r') = P psi / d + gd u
//   h_e = M^T w + Xi_s^T g'  (into hpos as above),   hstrain[s] += w (x) r + g' (x) t  (t = v[src] - v[dst], unstrained),
// reduced exactly as the first-order kernel reduces g_strain (S = 1: registers, LDS, one partial per block; S > 1: one wave
// reduction per row and a 9-lane atomic).  v or Xi may be NULL (zeros), hpos or hstrain may be NULL (not formed).
template <int LMAX, int PBC, bool STRAIN, class... SA>
__global__ __launch_bounds__(256) void edge_geometry_hvp_kernel(const float4* __restrict__ pos4,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ src, int64_t N,
                                                                const float* __restrict__ gY, const float* __restrict__ gd,
                                                                const float* __restrict__ gA, const float* __restrict__ v,
                                                                float* __restrict__ hpos,
                                                                const typename PbcArg<PBC>::type box, const SA... tail) {
  static_assert(sizeof...(SA) == (STRAIN ? 1 : 0), "the strained kernels take one StrainTangent, the others nothing");
  constexpr int NY = (LMAX + 1) * (LMAX + 1);
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float G[9];
  if constexpr (STRAIN) {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = 0.f;
  }
  for (int64_t i = wave0; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    if (b == e) continue;
    const float4 pi = pos4[i];
    // v[i]; the strained kernels take a NULL v as zeros, the others load unconditionally (the test folds away)
    const float vix = (!STRAIN || v) ? v[i * 3 + 0] : 0.f, viy = (!STRAIN || v) ? v[i * 3 + 1] : 0.f,
                viz = (!STRAIN || v) ? v[i * 3 + 2] : 0.f;
    const float invdeg = 1.0f / (float)(e - b);
    float ga[NY];
#pragma unroll
    for (int k = 1; k < NY; ++k) ga[k] = node_cotangent(gA, i * NY + k, invdeg);
    int srow = 0;
    float eps[9], xi[9];
    if constexpr (STRAIN) {
      const StrainTangent& sa = only(tail...);
      srow = row_structure(sa.st, i);
      load_strain(sa.st, srow, eps);
      load_strain_cotangent(sa.xi, srow, xi);
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int q = b + lane; q < e; q += 64) {
      const int j = src[q];
      EdgeVec ev;
      if (!edge_vec<PBC, STRAIN>(pos4[j], pi, box, eps, ev)) continue;
      edge_unit(ev);
      const float inv = ev.inv, x = ev.x, y = ev.y, z = ev.z;
      float g[NY];
#pragma unroll
      for (int k = 1; k < NY; ++k) g[k] = edge_cotangent(gY, (int64_t)q * NY + k, ga[k]);
      const float t0x = ((!STRAIN || v) ? v[(int64_t)j * 3 + 0] : 0.f) - vix;  // t (the strained kernels: before the strain)
      const float t0y = ((!STRAIN || v) ? v[(int64_t)j * 3 + 1] : 0.f) - viy;
      const float t0z = ((!STRAIN || v) ? v[(int64_t)j * 3 + 2] : 0.f) - viz;
      float tx = t0x, ty = t0y, tz = t0z;
      if constexpr (STRAIN) strain_tangent(eps, xi, ev.r0x, ev.r0y, ev.r0z, tx, ty, tz);
      const float dd = x * tx + y * ty + z * tz;
      const float dux = (tx - x * dd) * inv, duy = (ty - y * dd) * inv, duz = (tz - z * dd) * inv;
      float px = kS3 * g[1], py = kS3 * g[2], pz = kS3 * g[3];  // psi
      float wx = 0.f, wy = 0.f, wz = 0.f;                       // Q du
      if constexpr (LMAX == 2) {
        const float qxx = kS5 * (kS3 * g[8] - g[6]), qyy = -kS5 * (kS3 * g[8] + g[6]), qzz = 2.f * kS5 * g[6];
        const float qxy = kS5 * kS3 * g[4], qyz = kS5 * kS3 * g[5], qzx = kS5 * kS3 * g[7];
        px += qxx * x + qxy * y + qzx * z;
        py += qxy * x + qyy * y + qyz * z;
        pz += qzx * x + qyz * y + qzz * z;
        wx = qxx * dux + qxy * duy + qzx * duz;
        wy = qxy * dux + qyy * duy + qyz * duz;
        wz = qzx * dux + qyz * duy + qzz * duz;
      }
      const float up = x * px + y * py + z * pz;         // u . psi
      const float dp = dux * px + duy * py + duz * pz;   // du . psi
      const float uw = x * wx + y * wy + z * wz;         // u . Q du
      const float gdv = gd ? gd[q] : 0.f;
      const float c = gdv - up * inv, s = dd * inv * inv;
      // [P Q du - du (u . psi) - u (du . psi)] / d - (psi - u (u . psi)) dd / d^2 + gd du
      float hx = (wx - x * (uw + dp)) * inv + c * dux - (px - x * up) * s;
      float hy = (wy - y * (uw + dp)) * inv + c * duy - (py - y * up) * s;
      float hz = (wz - z * (uw + dp)) * inv + c * duz - (pz - z * up) * s;
      if constexpr (STRAIN) {
        // g' = grad phi at r': (psi - u (u . psi)) / d + gd u
        const float gx = (px - x * up) * inv + gdv * x, gy = (py - y * up) * inv + gdv * y,
                    gz = (pz - z * up) * inv + gdv * z;
        if (srow >= 0) {
          G[0] += hx * ev.r0x + gx * t0x; G[1] += hx * ev.r0y + gx * t0y; G[2] += hx * ev.r0z + gx * t0z;
          G[3] += hy * ev.r0x + gy * t0x; G[4] += hy * ev.r0y + gy * t0y; G[5] += hy * ev.r0z + gy * t0z;
          G[6] += hz * ev.r0x + gz * t0x; G[7] += hz * ev.r0y + gz * t0y; G[8] += hz * ev.r0z + gz * t0z;
        }
        // M^T w + Xi^T g'
        const float mx = hx + (eps[0] * hx + eps[3] * hy + eps[6] * hz) + (xi[0] * gx + xi[3] * gy + xi[6] * gz);
        const float my = hy + (eps[1] * hx + eps[4] * hy + eps[7] * hz) + (xi[1] * gx + xi[4] * gy + xi[7] * gz);
        const float mz = hz + (eps[2] * hx + eps[5] * hy + eps[8] * hz) + (xi[2] * gx + xi[5] * gy + xi[8] * gz);
        hx = mx; hy = my; hz = mz;
      }
      if (!STRAIN || hpos) atomic_add3(hpos + (int64_t)j * 3, hx, hy, hz);
      sx += hx; sy += hy; sz += hz;
    }
    wave_sum3(sx, sy, sz);
    if (lane == 0 && (!STRAIN || hpos)) atomic_add3(hpos + i * 3, -sx, -sy, -sz);
    if constexpr (STRAIN) {
      const StrainTangent& sa = only(tail...);
      if (sa.st.S > 1 && srow >= 0 && sa.hstrain) strain_row_flush(G, lane, sa.hstrain + (int64_t)srow * 9);
    }
  }
  if constexpr (STRAIN) {
    const StrainTangent& sa = only(tail...);
    if (sa.st.S == 1 && sa.hstrain) strain_block_flush(G, sa.hpart);
  }
}

}  // namespace e3

using namespace e3;

// one periodicity mode (box: the mode's kernel argument, validated by the caller); st: NULL = unstrained, else validated by
// the caller (g_strain [S,9], workspace of e3_edge_geometry_backward_strained_workspace_bytes when S = 1)
template <int PBC>
static int edge_geometry_backward(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                  const typename PbcArg<PBC>::type& b, const StrainArg* st, float* g_strain, float* gpart,
                                  void* stream) {
  if (!geometry_args_valid(N, lmax)) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (st) E3_HIP_CHECK(hipMemsetAsync(g_strain, 0, (size_t)st->S * 9 * sizeof(float), s));
  if (N == 0) return E3_OK;
  if (!pos4 || !rowptr || !src || !g_pos) return E3_ERR_INVALID_ARG;
  E3_HIP_CHECK(hipMemsetAsync(g_pos, 0, (size_t)N * 3 * sizeof(float), s));
  const int grid = wave_grid(N);
  if (!st) {
    auto kern = lmax == 1 ? edge_geometry_bwd_kernel<1, PBC, false> : edge_geometry_bwd_kernel<2, PBC, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d,
                       g_node_a, g_pos, b, StrainArg{nullptr, nullptr, 0}, nullptr, nullptr);
  } else {
    auto kern = lmax == 1 ? edge_geometry_bwd_kernel<1, PBC, true> : edge_geometry_bwd_kernel<2, PBC, true>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d,
                       g_node_a, g_pos, b, *st, g_strain, gpart);
    E3_HIP_CHECK(hipGetLastError());
    if (st->S == 1) hipLaunchKernelGGL(strain_partial_sum_kernel, dim3(1), dim3(576), 0, s, gpart, grid, g_strain);
  }
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}
// open (box NULL) or orthorhombic box
static int edge_geometry_backward(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                  const float* box, const StrainArg* st, float* g_strain, float* gpart, void* stream) {
  return dispatch_box(box, [&](auto mode, const PbcBox& b) {
    return edge_geometry_backward<decltype(mode)::value>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, b,
                                                         st, g_strain, gpart, stream);
  });
}

// the tangent in one periodicity mode (box: the mode's kernel argument, validated by the caller); sa: NULL = unstrained (v
// required), else the strain with its cotangent xi (v or xi required)
template <int PBC>
static int edge_geometry_jvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                             const typename PbcArg<PBC>::type& b, const StrainTangent* sa, void* stream) {
  if (sa ? !strained_args_valid(N, lmax, sa->st.eps, sa->st.S) || (!v && !sa->xi) : !geometry_args_valid(N, lmax))
    return E3_ERR_INVALID_ARG;
  if (N == 0 || (!d_edge_y && !d_edge_d && !d_node_a)) return E3_OK;
  if (!pos4 || !rowptr || !src || (!sa && !v)) return E3_ERR_INVALID_ARG;
  const dim3 grid(wave_grid(N));
  const hipStream_t s = (hipStream_t)stream;
  if (!sa) {
    auto kern = lmax == 1 ? edge_geometry_jvp_kernel<1, PBC, false> : edge_geometry_jvp_kernel<2, PBC, false>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, v, d_edge_y, d_edge_d, d_node_a, b);
  } else {
    auto kern = lmax == 1 ? edge_geometry_jvp_kernel<1, PBC, true, StrainTangent>
                          : edge_geometry_jvp_kernel<2, PBC, true, StrainTangent>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, v, d_edge_y, d_edge_d, d_node_a, b,
                       *sa);
  }
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// the Hessian in one periodicity mode (box: the mode's kernel argument, validated by the caller); sa: NULL = unstrained (v
// and h_pos required), else the strain with xi, h_strain and the S = 1 workspace (v or xi, and h_pos or h_strain, required).
// The grid is the one of the strained backward, so its workspace serves
template <int PBC>
static int edge_geometry_hvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                             float* h_pos, const typename PbcArg<PBC>::type& b, const StrainTangent* sa,
                             int64_t workspace_bytes, void* stream) {
  if (sa ? !strained_args_valid(N, lmax, sa->st.eps, sa->st.S) || (!v && !sa->xi) || (!h_pos && !sa->hstrain) ||
               (sa->hstrain && !strain_workspace_valid(sa->st.S, N, sa->hpart, workspace_bytes))
         : !geometry_args_valid(N, lmax) || !v || !h_pos)
    return E3_ERR_INVALID_ARG;
  if (N > 0 && (!rowptr || (src && !pos4))) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (sa && sa->hstrain) E3_HIP_CHECK(hipMemsetAsync(sa->hstrain, 0, (size_t)sa->st.S * 9 * sizeof(float), s));
  if (N == 0) return E3_OK;
  if (h_pos) E3_HIP_CHECK(hipMemsetAsync(h_pos, 0, (size_t)N * 3 * sizeof(float), s));
  if (!src) return E3_OK;  // a graph without edges has no src to hand over: every row is empty
  const int grid = wave_grid(N);
  if (!sa) {
    auto kern = lmax == 1 ? edge_geometry_hvp_kernel<1, PBC, false> : edge_geometry_hvp_kernel<2, PBC, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d,
                       g_node_a, v, h_pos, b);
  } else {
    auto kern = lmax == 1 ? edge_geometry_hvp_kernel<1, PBC, true, StrainTangent>
                          : edge_geometry_hvp_kernel<2, PBC, true, StrainTangent>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d,
                       g_node_a, v, h_pos, b, *sa);
  }
  E3_HIP_CHECK(hipGetLastError());
  if (sa && sa->st.S == 1 && sa->hstrain) {
    hipLaunchKernelGGL(strain_partial_sum_kernel, dim3(1), dim3(576), 0, s, (const float*)sa->hpart, grid, sa->hstrain);
    E3_HIP_CHECK(hipGetLastError());
  }
  return E3_OK;
}

extern "C" {

int e3_edge_geometry_hvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                         const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v, float* h_pos,
                         void* stream) {
  return edge_geometry_hvp<kOpen>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, make_box(nullptr),
                                  nullptr, 0, stream);
}

int e3_edge_geometry_hvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                             const float* v, float* h_pos, void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return edge_geometry_hvp<kBox>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, make_box(box), nullptr,
                                 0, stream);
}

int e3_edge_geometry_hvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                              const float* v, float* h_pos, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_hvp<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, c, nullptr, 0, stream);
}

int e3_edge_geometry_jvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax, const float* v,
                         float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream) {
  return edge_geometry_jvp<kOpen>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, make_box(nullptr), nullptr,
                                  stream);
}

int e3_edge_geometry_jvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                             void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return edge_geometry_jvp<kBox>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, make_box(box), nullptr,
                                 stream);
}

int e3_edge_geometry_jvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                              void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_jvp<kCell>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, c, nullptr, stream);
}

int e3_edge_geometry_jvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S, const float* v,
                                  const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream) {
  if (box && !box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  const StrainTangent sa = {{strain, structure, S}, xi, nullptr, nullptr};
  return dispatch_box(box, [&](auto mode, const PbcBox& b) {
    return edge_geometry_jvp<decltype(mode)::value>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, b, &sa,
                                                    stream);
  });
}

int e3_edge_geometry_jvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* v, const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a,
                                       void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  const StrainTangent sa = {{strain, structure, S}, xi, nullptr, nullptr};
  return edge_geometry_jvp<kCell>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, c, &sa, stream);
}

int e3_edge_geometry_hvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                  const float* xi, float* h_pos, float* h_strain, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (box && !box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  const StrainTangent sa = {{strain, structure, S}, xi, h_strain, (float*)workspace};
  return dispatch_box(box, [&](auto mode, const PbcBox& b) {
    return edge_geometry_hvp<decltype(mode)::value>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, b,
                                                    &sa, workspace_bytes, stream);
  });
}

int e3_edge_geometry_hvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                       const float* xi, float* h_pos, float* h_strain, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  const StrainTangent sa = {{strain, structure, S}, xi, h_strain, (float*)workspace};
  return edge_geometry_hvp<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, c, &sa,
                                  workspace_bytes, stream);
}

int e3_edge_geometry_backward(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                              void* stream) {
  return edge_geometry_backward(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, nullptr, nullptr, nullptr,
                                nullptr, stream);
}

int e3_edge_geometry_backward_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float box[3], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                                  float* g_pos, void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return edge_geometry_backward(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, box, nullptr, nullptr,
                                nullptr, stream);
}

int64_t e3_edge_geometry_backward_strained_workspace_bytes(int64_t N) {
  if (N < 0) return -1;
  return N == 0 ? 0 : (int64_t)wave_grid(N) * 9 * (int64_t)sizeof(float);
}

int e3_edge_geometry_backward_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float* box, const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                       float* g_strain, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!strained_args_valid(N, lmax, strain, S) || !g_strain || (box && !box_valid(box, 0.0f))) return E3_ERR_INVALID_ARG;
  if (!strain_workspace_valid(S, N, workspace, workspace_bytes)) return E3_ERR_INVALID_ARG;
  const StrainArg st = {strain, structure, S};
  return edge_geometry_backward(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, box, &st, g_strain,
                                (float*)workspace, stream);
}

int e3_edge_geometry_backward_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                   const float cell[9], const float* g_edge_y, const float* g_edge_d,
                                   const float* g_node_a, float* g_pos, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_backward<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, c, nullptr, nullptr,
                                       nullptr, stream);
}

int e3_edge_geometry_backward_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N,
                                            int lmax, const float cell[9], const float* strain, const int32_t* structure,
                                            int S, const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                                            float* g_pos, float* g_strain, void* workspace, int64_t workspace_bytes,
                                            void* stream) {
  PbcCell c;
  if (!strained_args_valid(N, lmax, strain, S) || !g_strain || !make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  if (!strain_workspace_valid(S, N, workspace, workspace_bytes)) return E3_ERR_INVALID_ARG;
  const StrainArg st = {strain, structure, S};
  return edge_geometry_backward<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, c, &st, g_strain,
                                       (float*)workspace, stream);
}

}  // extern "C"
