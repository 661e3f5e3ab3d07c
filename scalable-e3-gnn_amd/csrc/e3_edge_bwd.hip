// Backward of the edge / node stages around the tensor product (forward: e3_edge_ops.hip) -- what the force head
// (-dE/dpos, BASELINE.json configs[3]) and parameter gradients through a whole SEGNN layer need besides the tensor
// product's own backward (e3_l1tp_backward / e3_tp_backward).  Builder-defined stages; the
// reference's contract for its operator is plain torch autograd (l1_tensor_prod.py:234-299), and these kernels are that
// for the stages it does not contain.  fp32, one wave per CSR row where a row is reduced, HBM-bound streaming kernels.
#include "e3_common.h"

#include <algorithm>

namespace e3 {

constexpr float kS3 = 1.7320508075688772f, kS5 = 2.2360679774997896f;

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
    for (int k = 1; k < NY; ++k) ga[k] = gA ? gA[i * NY + k] * invdeg : 0.f;
    int srow = 0;
    float eps[9];
    if constexpr (STRAIN) {
      srow = row_structure(st, i);
      load_strain(st, srow, eps);
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int q = b + lane; q < e; q += 64) {
      const int j = src[q];
      const float4 pj = pos4[j];
      float rx, ry, rz;
      edge_rel<PBC>(pj, pi, box, rx, ry, rz);
      const float r0x = rx, r0y = ry, r0z = rz;
      if constexpr (STRAIN) apply_strain(eps, rx, ry, rz);
      const float d = sqrtf(rx * rx + ry * ry + rz * rz);
      if (!(d > 0.f)) continue;
      const float inv = 1.0f / d;
      const float x = rx * inv, y = ry * inv, z = rz * inv;
      float g[NY];
#pragma unroll
      for (int k = 1; k < NY; ++k) g[k] = (gY ? gY[(int64_t)q * NY + k] : 0.f) + ga[k];
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
          G[0] += gx * r0x; G[1] += gx * r0y; G[2] += gx * r0z;
          G[3] += gy * r0x; G[4] += gy * r0y; G[5] += gy * r0z;
          G[6] += gz * r0x; G[7] += gz * r0y; G[8] += gz * r0z;
        }
        const float tx = gx + (eps[0] * gx + eps[3] * gy + eps[6] * gz);
        const float ty = gy + (eps[1] * gx + eps[4] * gy + eps[7] * gz);
        const float tz = gz + (eps[2] * gx + eps[5] * gy + eps[8] * gz);
        gx = tx; gy = ty; gz = tz;
      } else {
        (void)r0x; (void)r0y; (void)r0z;
      }
      atomicAdd(gpos + (int64_t)j * 3 + 0, gx);
      atomicAdd(gpos + (int64_t)j * 3 + 1, gy);
      atomicAdd(gpos + (int64_t)j * 3 + 2, gz);
      sx += gx; sy += gy; sz += gz;
    }
    for (int o = 32; o > 0; o >>= 1) {
      sx += __shfl_xor(sx, o);
      sy += __shfl_xor(sy, o);
      sz += __shfl_xor(sz, o);
    }
    if (lane == 0) {
      atomicAdd(gpos + i * 3 + 0, -sx);
      atomicAdd(gpos + i * 3 + 1, -sy);
      atomicAdd(gpos + i * 3 + 2, -sz);
    }
    if constexpr (STRAIN) {
      if (st.S > 1 && srow >= 0) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
          if (lane == k) v = G[k];
          G[k] = 0.f;
        }
        if (lane < 9) atomicAdd(gstrain + (int64_t)srow * 9 + lane, v);
      }
    }
  }
  if constexpr (STRAIN) {
    if (st.S == 1) {
      __shared__ float part[4][9];
      const int w = threadIdx.x >> 6;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
        if (lane == 0) part[w][k] = G[k];
      }
      __syncthreads();
      if (threadIdx.x < 9)
        gpart[(int64_t)blockIdx.x * 9 + threadIdx.x] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    }
  }
}

// G[k] = sum of the per-block partials gpart[p, k] of edge_geometry_bwd_kernel (S = 1): one wave per component, lanes over
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

// m[e] = [h[dst] | h[src] | extra[e]]:  g_h[dst] += sum over the row of gm[e, :D] (one atomic per row and column),
// g_h[src[e]] += gm[e, D:2D] (atomics), g_extra[e] = gm[e, 2D:]
__global__ __launch_bounds__(256) void gather_concat_bwd_kernel(const float* __restrict__ gm, int64_t ld_gm, int D,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ src, int64_t N, int n_extra,
                                                                float* __restrict__ gh, int64_t ld_gh,
                                                                float* __restrict__ gextra) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    if (b == e) continue;
    for (int c = lane; c < D; c += 64) {
      float acc = 0.f;
      for (int q = b; q < e; ++q) {
        const float* g = gm + (int64_t)q * ld_gm;
        acc += g[c];
        atomicAdd(gh + (int64_t)src[q] * ld_gh + c, g[D + c]);
      }
      atomicAdd(gh + i * ld_gh + c, acc);
    }
    if (gextra)
      for (int q = b; q < e; ++q)
        if (lane < n_extra) gextra[(int64_t)q * n_extra + lane] = gm[(int64_t)q * ld_gm + 2 * D + lane];
  }
}

struct GateBlocksB {
  int nblocks;
  int l[8], mul[8];
};
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }

// out = [silu(s) | sigmoid(g_k) v_k]:  d silu = sig (1 + s (1 - sig));  g_v = sig(g) gout;  g_g = sig (1 - sig) sum_m v gout
// One thread per INPUT column (scalar, gate or gated component): the gate column sums over its channel's components.
__global__ __launch_bounds__(256) void gate_blocks_bwd_kernel(const float* __restrict__ in, int64_t ld_in,
                                                              const float* __restrict__ gout, int64_t ld_go,
                                                              float* __restrict__ gin, int64_t ld_gi, int64_t B, int ns,
                                                              int ngates, int W, GateBlocksB gb) {
  const int WI = W + ngates;  // input width: [ns | ngates | wide]
  const int64_t total = B * (int64_t)WI;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / WI;
    const int c = (int)(t - row * WI);
    const float* x = in + row * ld_in;
    const float* go = gout + row * ld_go;
    float v;
    if (c < ns) {
      const float s = x[c], sg = sigm(s);
      v = go[c] * sg * (1.f + s * (1.f - sg));
    } else if (c < ns + ngates) {
      // gate k: find its block and channel
      int k = c - ns, bi = 0, col0 = ns;  // col0: first OUTPUT column of block bi
      while (k >= gb.mul[bi]) { k -= gb.mul[bi]; col0 += gb.mul[bi] * (2 * gb.l[bi] + 1); ++bi; }
      const int w = 2 * gb.l[bi] + 1;
      float acc = 0.f;
      for (int m = 0; m < w; ++m) acc += x[ngates + col0 + k * w + m] * go[col0 + k * w + m];
      const float sg = sigm(x[c]);
      v = acc * sg * (1.f - sg);
    } else {
      const int oc = c - ngates;  // output column
      int rem = oc - ns, g0 = 0, bi = 0;
      while (rem >= gb.mul[bi] * (2 * gb.l[bi] + 1)) { rem -= gb.mul[bi] * (2 * gb.l[bi] + 1); g0 += gb.mul[bi]; ++bi; }
      const int k = rem / (2 * gb.l[bi] + 1);
      v = sigm(x[ns + g0 + k]) * go[oc];
    }
    gin[row * ld_gi + c] = v;
  }
}

// Backward of gate_blocks_bwd_kernel (include/e3gnn.h, e3_gate_blocks_backward2): ct = the cotangent of gin.  Same thread
// mapping, one thread per INPUT column; a scalar / gated thread also writes the output-gradient cotangent of its own column.
//   silu'' = sig' (2 + s (1 - 2 sig)),  sig' = sig (1 - sig),  sig'' = sig' (1 - 2 sig)
__global__ __launch_bounds__(256) void gate_blocks_bwd2_kernel(const float* __restrict__ in, int64_t ld_in,
                                                               const float* __restrict__ gout, int64_t ld_go,
                                                               const float* __restrict__ ct, int64_t ld_ct,
                                                               float* __restrict__ cgo, int64_t ld_cgo,
                                                               float* __restrict__ cin, int64_t ld_cin, int64_t B, int ns,
                                                               int ngates, int W, GateBlocksB gb) {
  const int WI = W + ngates;  // input width: [ns | ngates | wide]
  const int64_t total = B * (int64_t)WI;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / WI;
    const int c = (int)(t - row * WI);
    const float* x = in + row * ld_in;
    const float* go = gout + row * ld_go;
    const float* cr = ct + row * ld_ct;
    float vin;
    if (c < ns) {
      const float s = x[c], sg = sigm(s), dsg = sg * (1.f - sg);
      if (cgo) cgo[row * ld_cgo + c] = cr[c] * sg * (1.f + s * (1.f - sg));
      vin = cr[c] * go[c] * dsg * (2.f + s * (1.f - 2.f * sg));
    } else if (c < ns + ngates) {
      int k = c - ns, bi = 0, col0 = ns;  // col0: first OUTPUT column of block bi
      while (k >= gb.mul[bi]) { k -= gb.mul[bi]; col0 += gb.mul[bi] * (2 * gb.l[bi] + 1); ++bi; }
      const int w = 2 * gb.l[bi] + 1;
      float acc_c = 0.f, acc_v = 0.f;
      for (int m = 0; m < w; ++m) {
        const float g = go[col0 + k * w + m];
        acc_c += cr[ngates + col0 + k * w + m] * g;
        acc_v += x[ngates + col0 + k * w + m] * g;
      }
      const float sg = sigm(x[c]), dsg = sg * (1.f - sg);
      vin = dsg * acc_c + dsg * (1.f - 2.f * sg) * cr[c] * acc_v;
    } else {
      const int oc = c - ngates;  // output column
      int rem = oc - ns, g0 = 0, bi = 0;
      while (rem >= gb.mul[bi] * (2 * gb.l[bi] + 1)) { rem -= gb.mul[bi] * (2 * gb.l[bi] + 1); g0 += gb.mul[bi]; ++bi; }
      const int gc = ns + g0 + rem / (2 * gb.l[bi] + 1);  // the gate column of this channel
      const float sg = sigm(x[gc]), dsg = sg * (1.f - sg);
      if (cgo) cgo[row * ld_cgo + oc] = sg * cr[c] + dsg * cr[gc] * x[c];
      vin = dsg * cr[gc] * go[oc];
    }
    if (cin) cin[row * ld_cin + c] = vin;
  }
}

// Tangent of the edge geometry along a displacement field v [N,3] (include/e3gnn.h, e3_edge_geometry_jvp): the backward above
// is linear in (gY, gd, gA), so this is its backward w.r.t. those three.  t = v[src] - v[dst];  du = (t - u (u . t)) / d;
//   dY1 = sqrt3 du,  dY2 = sqrt5 (db/du) du  (b as above),  dd = u . t,  dA_i = (1 / deg_i) sum over the row of dY_e.
// One wave per row, lanes over its edges; dA: per-lane sums in edge order, then a fixed butterfly -- no atomics.
// STRAIN (e3_edge_geometry_jvp_strained): u and d are those of r' = (I + eps_s) r and the tangent of r' is
// t' = (I + eps_s) t + Xi_s r, Xi [S,9] the cotangent of g_strain (r unstrained); v or Xi may be NULL (zeros).  eps_s and Xi_s
// are read once per row with a wave-uniform structure id; a row outside [0, S) has eps = Xi = 0.
//
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
    float vix, viy, viz;
    if constexpr (STRAIN) {
      vix = v ? v[i * 3 + 0] : 0.f; viy = v ? v[i * 3 + 1] : 0.f; viz = v ? v[i * 3 + 2] : 0.f;
    } else {
      vix = v[i * 3 + 0]; viy = v[i * 3 + 1]; viz = v[i * 3 + 2];
    }
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
      const float4 pj = pos4[j];
      float rx, ry, rz;
      edge_rel<PBC>(pj, pi, box, rx, ry, rz);
      const float r0x = rx, r0y = ry, r0z = rz;
      if constexpr (STRAIN) apply_strain(eps, rx, ry, rz);
      const float d = sqrtf(rx * rx + ry * ry + rz * rz);
      float o[NY], ddv = 0.f;
#pragma unroll
      for (int k = 0; k < NY; ++k) o[k] = 0.f;
      if (d > 0.f) {
        const float inv = 1.0f / d;
        const float x = rx * inv, y = ry * inv, z = rz * inv;
        float tx, ty, tz;
        if constexpr (STRAIN) {
          tx = (v ? v[(int64_t)j * 3 + 0] : 0.f) - vix;
          ty = (v ? v[(int64_t)j * 3 + 1] : 0.f) - viy;
          tz = (v ? v[(int64_t)j * 3 + 2] : 0.f) - viz;
          strain_tangent(eps, xi, r0x, r0y, r0z, tx, ty, tz);
        } else {
          (void)r0x; (void)r0y; (void)r0z;
          tx = v[(int64_t)j * 3 + 0] - vix; ty = v[(int64_t)j * 3 + 1] - viy; tz = v[(int64_t)j * 3 + 2] - viz;
        }
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
    float vix, viy, viz;
    if constexpr (STRAIN) {
      vix = v ? v[i * 3 + 0] : 0.f; viy = v ? v[i * 3 + 1] : 0.f; viz = v ? v[i * 3 + 2] : 0.f;
    } else {
      vix = v[i * 3 + 0]; viy = v[i * 3 + 1]; viz = v[i * 3 + 2];
    }
    const float invdeg = 1.0f / (float)(e - b);
    float ga[NY];
#pragma unroll
    for (int k = 1; k < NY; ++k) ga[k] = gA ? gA[i * NY + k] * invdeg : 0.f;
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
      const float4 pj = pos4[j];
      float rx, ry, rz;
      edge_rel<PBC>(pj, pi, box, rx, ry, rz);
      const float r0x = rx, r0y = ry, r0z = rz;
      if constexpr (STRAIN) apply_strain(eps, rx, ry, rz);
      const float d = sqrtf(rx * rx + ry * ry + rz * rz);
      if (!(d > 0.f)) continue;
      const float inv = 1.0f / d;
      const float x = rx * inv, y = ry * inv, z = rz * inv;
      float g[NY];
#pragma unroll
      for (int k = 1; k < NY; ++k) g[k] = (gY ? gY[(int64_t)q * NY + k] : 0.f) + ga[k];
      float tx, ty, tz;
      float t0x = 0.f, t0y = 0.f, t0z = 0.f;  // STRAIN: the unstrained t
      if constexpr (STRAIN) {
        tx = t0x = (v ? v[(int64_t)j * 3 + 0] : 0.f) - vix;
        ty = t0y = (v ? v[(int64_t)j * 3 + 1] : 0.f) - viy;
        tz = t0z = (v ? v[(int64_t)j * 3 + 2] : 0.f) - viz;
        strain_tangent(eps, xi, r0x, r0y, r0z, tx, ty, tz);
      } else {
        (void)r0x; (void)r0y; (void)r0z; (void)t0x; (void)t0y; (void)t0z;
        tx = v[(int64_t)j * 3 + 0] - vix; ty = v[(int64_t)j * 3 + 1] - viy; tz = v[(int64_t)j * 3 + 2] - viz;
      }
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
          G[0] += hx * r0x + gx * t0x; G[1] += hx * r0y + gx * t0y; G[2] += hx * r0z + gx * t0z;
          G[3] += hy * r0x + gy * t0x; G[4] += hy * r0y + gy * t0y; G[5] += hy * r0z + gy * t0z;
          G[6] += hz * r0x + gz * t0x; G[7] += hz * r0y + gz * t0y; G[8] += hz * r0z + gz * t0z;
        }
        // M^T w + Xi^T g'
        const float mx = hx + (eps[0] * hx + eps[3] * hy + eps[6] * hz) + (xi[0] * gx + xi[3] * gy + xi[6] * gz);
        const float my = hy + (eps[1] * hx + eps[4] * hy + eps[7] * hz) + (xi[1] * gx + xi[4] * gy + xi[7] * gz);
        const float mz = hz + (eps[2] * hx + eps[5] * hy + eps[8] * hz) + (xi[2] * gx + xi[5] * gy + xi[8] * gz);
        hx = mx; hy = my; hz = mz;
        if (hpos) {
          atomicAdd(hpos + (int64_t)j * 3 + 0, hx);
          atomicAdd(hpos + (int64_t)j * 3 + 1, hy);
          atomicAdd(hpos + (int64_t)j * 3 + 2, hz);
        }
      } else {
        atomicAdd(hpos + (int64_t)j * 3 + 0, hx);
        atomicAdd(hpos + (int64_t)j * 3 + 1, hy);
        atomicAdd(hpos + (int64_t)j * 3 + 2, hz);
      }
      sx += hx; sy += hy; sz += hz;
    }
    for (int o = 32; o > 0; o >>= 1) {
      sx += __shfl_xor(sx, o);
      sy += __shfl_xor(sy, o);
      sz += __shfl_xor(sz, o);
    }
    if (lane == 0 && (!STRAIN || hpos)) {
      atomicAdd(hpos + i * 3 + 0, -sx);
      atomicAdd(hpos + i * 3 + 1, -sy);
      atomicAdd(hpos + i * 3 + 2, -sz);
    }
    if constexpr (STRAIN) {
      const StrainTangent& sa = only(tail...);
      if (sa.st.S > 1 && srow >= 0 && sa.hstrain) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
          if (lane == k) a = G[k];
          G[k] = 0.f;
        }
        if (lane < 9) atomicAdd(sa.hstrain + (int64_t)srow * 9 + lane, a);
      }
    }
  }
  if constexpr (STRAIN) {
    const StrainTangent& sa = only(tail...);
    if (sa.st.S == 1 && sa.hstrain) {
      __shared__ float part[4][9];
      const int w = threadIdx.x >> 6;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        for (int o = 32; o > 0; o >>= 1) G[k] += __shfl_xor(G[k], o);
        if (lane == 0) part[w][k] = G[k];
      }
      __syncthreads();
      if (threadIdx.x < 9)
        sa.hpart[(int64_t)blockIdx.x * 9 + threadIdx.x] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    }
  }
}

// agg[i] = sum over the row of msg[e]  ->  gmsg[e] = gagg[dst(e)]
__global__ __launch_bounds__(256) void segment_sum_bwd_kernel(const float* __restrict__ gagg, int64_t ld_ga,
                                                              const int32_t* __restrict__ rowptr, int64_t N, int D,
                                                              float* __restrict__ gmsg, int64_t ld_gm) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave0; i < N; i += nw) {
    const int b = rowptr[i], e = rowptr[i + 1];
    for (int c = lane; c < D; c += 64) {
      const float v = gagg[i * ld_ga + c];
      for (int q = b; q < e; ++q) gmsg[(int64_t)q * ld_gm + c] = v;
    }
  }
}

static inline int wave_grid_b(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 256 * 16)); }

}  // namespace e3

using namespace e3;

// one periodicity mode (box: the mode's kernel argument, validated by the caller); st: NULL = unstrained, else validated by
// the caller (g_strain [S,9], workspace of e3_edge_geometry_backward_strained_workspace_bytes when S = 1)
template <int PBC>
static int edge_geometry_backward(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                  const typename PbcArg<PBC>::type& b, const StrainArg* st, float* g_strain, float* gpart,
                                  void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2)) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (st) E3_HIP_CHECK(hipMemsetAsync(g_strain, 0, (size_t)st->S * 9 * sizeof(float), s));
  if (N == 0) return E3_OK;
  if (!pos4 || !rowptr || !src || !g_pos) return E3_ERR_INVALID_ARG;
  E3_HIP_CHECK(hipMemsetAsync(g_pos, 0, (size_t)N * 3 * sizeof(float), s));
  const int grid = wave_grid_b(N);
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
  const PbcBox b = make_box(box);
  return box ? edge_geometry_backward<kBox>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, b, st,
                                            g_strain, gpart, stream)
             : edge_geometry_backward<kOpen>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, b, st,
                                             g_strain, gpart, stream);
}

// one periodicity mode (box: the mode's kernel argument, validated by the caller)
template <int PBC>
static int edge_geometry_jvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                             const typename PbcArg<PBC>::type& b, void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2)) return E3_ERR_INVALID_ARG;
  if (N == 0 || (!d_edge_y && !d_edge_d && !d_node_a)) return E3_OK;
  if (!pos4 || !rowptr || !src || !v) return E3_ERR_INVALID_ARG;
  auto kern = lmax == 1 ? edge_geometry_jvp_kernel<1, PBC, false> : edge_geometry_jvp_kernel<2, PBC, false>;
  hipLaunchKernelGGL(kern, dim3(wave_grid_b(N)), dim3(256), 0, (hipStream_t)stream, (const float4*)pos4, rowptr, src, N, v,
                     d_edge_y, d_edge_d, d_node_a, b);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// the strained tangent in one periodicity mode (box: the mode's kernel argument, validated by the caller)
template <int PBC>
static int edge_geometry_jvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                      const float* strain, const int32_t* structure, int S, const float* v, const float* xi,
                                      float* d_edge_y, float* d_edge_d, float* d_node_a,
                                      const typename PbcArg<PBC>::type& b, void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2) || !strain || S < 1 || (!v && !xi)) return E3_ERR_INVALID_ARG;
  if (N == 0 || (!d_edge_y && !d_edge_d && !d_node_a)) return E3_OK;
  if (!pos4 || !rowptr || !src) return E3_ERR_INVALID_ARG;
  auto kern = lmax == 1 ? edge_geometry_jvp_kernel<1, PBC, true, StrainTangent>
                        : edge_geometry_jvp_kernel<2, PBC, true, StrainTangent>;
  hipLaunchKernelGGL(kern, dim3(wave_grid_b(N)), dim3(256), 0, (hipStream_t)stream, (const float4*)pos4, rowptr, src, N, v,
                     d_edge_y, d_edge_d, d_node_a, b, StrainTangent{{strain, structure, S}, xi, nullptr, nullptr});
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// one periodicity mode (box: the mode's kernel argument, validated by the caller)
template <int PBC>
static int edge_geometry_hvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                             float* h_pos, const typename PbcArg<PBC>::type& b, void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2) || !v || !h_pos) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!rowptr || (src && !pos4)) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  E3_HIP_CHECK(hipMemsetAsync(h_pos, 0, (size_t)N * 3 * sizeof(float), s));
  if (!src) return E3_OK;  // a graph without edges has no src to hand over: every row is empty
  auto kern = lmax == 1 ? edge_geometry_hvp_kernel<1, PBC, false> : edge_geometry_hvp_kernel<2, PBC, false>;
  hipLaunchKernelGGL(kern, dim3(wave_grid_b(N)), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d,
                     g_node_a, v, h_pos, b);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// the strained Hessian in one periodicity mode (box: the mode's kernel argument, validated by the caller); the grid is the
// one of the strained backward, so its workspace serves
template <int PBC>
static int edge_geometry_hvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                      const float* strain, const int32_t* structure, int S, const float* g_edge_y,
                                      const float* g_edge_d, const float* g_node_a, const float* v, const float* xi,
                                      float* h_pos, float* h_strain, void* workspace, int64_t workspace_bytes,
                                      const typename PbcArg<PBC>::type& b, void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2) || !strain || S < 1 || (!v && !xi) || (!h_pos && !h_strain))
    return E3_ERR_INVALID_ARG;
  if (S == 1 && N > 0 && h_strain &&
      (!workspace || workspace_bytes < e3_edge_geometry_backward_strained_workspace_bytes(N)))
    return E3_ERR_INVALID_ARG;
  if (N > 0 && (!rowptr || (src && !pos4))) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (h_strain) E3_HIP_CHECK(hipMemsetAsync(h_strain, 0, (size_t)S * 9 * sizeof(float), s));
  if (N == 0) return E3_OK;
  if (h_pos) E3_HIP_CHECK(hipMemsetAsync(h_pos, 0, (size_t)N * 3 * sizeof(float), s));
  if (!src) return E3_OK;  // a graph without edges has no src to hand over: every row is empty
  const int grid = wave_grid_b(N);
  auto kern = lmax == 1 ? edge_geometry_hvp_kernel<1, PBC, true, StrainTangent>
                        : edge_geometry_hvp_kernel<2, PBC, true, StrainTangent>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, (const float4*)pos4, rowptr, src, N, g_edge_y, g_edge_d, g_node_a, v,
                     h_pos, b, StrainTangent{{strain, structure, S}, xi, h_strain, (float*)workspace});
  E3_HIP_CHECK(hipGetLastError());
  if (S == 1 && h_strain) {
    hipLaunchKernelGGL(strain_partial_sum_kernel, dim3(1), dim3(576), 0, s, (const float*)workspace, grid, h_strain);
    E3_HIP_CHECK(hipGetLastError());
  }
  return E3_OK;
}

extern "C" {

int e3_edge_geometry_hvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                         const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v, float* h_pos,
                         void* stream) {
  return edge_geometry_hvp<kOpen>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, make_box(nullptr),
                                  stream);
}

int e3_edge_geometry_hvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                             const float* v, float* h_pos, void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return edge_geometry_hvp<kBox>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, make_box(box), stream);
}

int e3_edge_geometry_hvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* g_edge_y, const float* g_edge_d, const float* g_node_a,
                              const float* v, float* h_pos, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_hvp<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, v, h_pos, c, stream);
}

int e3_edge_geometry_jvp(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax, const float* v,
                         float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream) {
  return edge_geometry_jvp<kOpen>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, make_box(nullptr), stream);
}

int e3_edge_geometry_jvp_pbc(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                             const float box[3], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                             void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return edge_geometry_jvp<kBox>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, make_box(box), stream);
}

int e3_edge_geometry_jvp_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                              const float cell[9], const float* v, float* d_edge_y, float* d_edge_d, float* d_node_a,
                              void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_jvp<kCell>(pos4, rowptr, src, N, lmax, v, d_edge_y, d_edge_d, d_node_a, c, stream);
}

int e3_edge_geometry_jvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S, const float* v,
                                  const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a, void* stream) {
  if (box && !box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  const PbcBox b = make_box(box);
  return box ? edge_geometry_jvp_strained<kBox>(pos4, rowptr, src, N, lmax, strain, structure, S, v, xi, d_edge_y, d_edge_d,
                                                d_node_a, b, stream)
             : edge_geometry_jvp_strained<kOpen>(pos4, rowptr, src, N, lmax, strain, structure, S, v, xi, d_edge_y, d_edge_d,
                                                 d_node_a, b, stream);
}

int e3_edge_geometry_jvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* v, const float* xi, float* d_edge_y, float* d_edge_d, float* d_node_a,
                                       void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_jvp_strained<kCell>(pos4, rowptr, src, N, lmax, strain, structure, S, v, xi, d_edge_y, d_edge_d,
                                           d_node_a, c, stream);
}

int e3_edge_geometry_hvp_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                  const float* box, const float* strain, const int32_t* structure, int S,
                                  const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                  const float* xi, float* h_pos, float* h_strain, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (box && !box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  const PbcBox b = make_box(box);
  return box ? edge_geometry_hvp_strained<kBox>(pos4, rowptr, src, N, lmax, strain, structure, S, g_edge_y, g_edge_d,
                                                g_node_a, v, xi, h_pos, h_strain, workspace, workspace_bytes, b, stream)
             : edge_geometry_hvp_strained<kOpen>(pos4, rowptr, src, N, lmax, strain, structure, S, g_edge_y, g_edge_d,
                                                 g_node_a, v, xi, h_pos, h_strain, workspace, workspace_bytes, b, stream);
}

int e3_edge_geometry_hvp_strained_cell(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float cell[9], const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, const float* v,
                                       const float* xi, float* h_pos, float* h_strain, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return edge_geometry_hvp_strained<kCell>(pos4, rowptr, src, N, lmax, strain, structure, S, g_edge_y, g_edge_d, g_node_a,
                                           v, xi, h_pos, h_strain, workspace, workspace_bytes, c, stream);
}

int e3_gate_blocks_backward2(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, const float* c,
                             int64_t ld_c, float* cot_g_out, int64_t ld_cgout, float* cot_in, int64_t ld_cin, int64_t B,
                             int ns, int nblocks, const int32_t* ls, const int32_t* muls, void* stream) {
  if (B < 0 || ns < 0 || nblocks < 0 || nblocks > 8 || (nblocks > 0 && (!ls || !muls))) return E3_ERR_INVALID_ARG;
  GateBlocksB gb;
  gb.nblocks = nblocks;
  int ngates = 0, wide = 0;
  for (int i = 0; i < 8; ++i) { gb.l[i] = 0; gb.mul[i] = 1 << 30; }
  for (int i = 0; i < nblocks; ++i) {
    if (ls[i] < 0 || ls[i] > 2 || muls[i] < 0) return E3_ERR_INVALID_ARG;
    gb.l[i] = ls[i]; gb.mul[i] = muls[i];
    ngates += muls[i];
    wide += muls[i] * (2 * ls[i] + 1);
  }
  const int W = ns + wide;
  if (ld_in < W + ngates || ld_gout < W || ld_c < W + ngates || (cot_g_out && ld_cgout < W) ||
      (cot_in && ld_cin < W + ngates))
    return E3_ERR_INVALID_ARG;
  if (B == 0 || W == 0 || (!cot_g_out && !cot_in)) return E3_OK;
  if (!in || !g_out || !c) return E3_ERR_INVALID_ARG;
  const int64_t total = B * (int64_t)(W + ngates);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(gate_blocks_bwd2_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, g_out, ld_gout, c,
                     ld_c, cot_g_out, ld_cgout, cot_in, ld_cin, B, ns, ngates, W, gb);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
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
  return N == 0 ? 0 : (int64_t)wave_grid_b(N) * 9 * (int64_t)sizeof(float);
}

int e3_edge_geometry_backward_strained(const float* pos4, const int32_t* rowptr, const int32_t* src, int64_t N, int lmax,
                                       const float* box, const float* strain, const int32_t* structure, int S,
                                       const float* g_edge_y, const float* g_edge_d, const float* g_node_a, float* g_pos,
                                       float* g_strain, void* workspace, int64_t workspace_bytes, void* stream) {
  if (N < 0 || (lmax != 1 && lmax != 2) || !strain || S < 1 || !g_strain || (box && !box_valid(box, 0.0f)))
    return E3_ERR_INVALID_ARG;
  if (S == 1 && N > 0 && (!workspace || workspace_bytes < e3_edge_geometry_backward_strained_workspace_bytes(N)))
    return E3_ERR_INVALID_ARG;
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
  if (N < 0 || (lmax != 1 && lmax != 2) || !strain || S < 1 || !g_strain || !make_cell(cell, 0.0f, &c))
    return E3_ERR_INVALID_ARG;
  if (S == 1 && N > 0 && (!workspace || workspace_bytes < e3_edge_geometry_backward_strained_workspace_bytes(N)))
    return E3_ERR_INVALID_ARG;
  const StrainArg st = {strain, structure, S};
  return edge_geometry_backward<kCell>(pos4, rowptr, src, N, lmax, g_edge_y, g_edge_d, g_node_a, g_pos, c, &st, g_strain,
                                       (float*)workspace, stream);
}

int e3_gather_concat_backward(const float* g_out, int64_t ld_gout, int D, const int32_t* rowptr, const int32_t* src,
                              int64_t N, int n_extra, float* g_h, int64_t ld_gh, float* g_extra, void* stream) {
  if (N < 0 || D <= 0 || n_extra < 0 || n_extra > 64 || ld_gout < 2 * D + n_extra || ld_gh < D) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!g_out || !rowptr || !src || !g_h) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  E3_HIP_CHECK(hipMemset2DAsync(g_h, (size_t)ld_gh * 4, 0, (size_t)D * 4, (size_t)N, s));
  hipLaunchKernelGGL(gather_concat_bwd_kernel, dim3(wave_grid_b(N)), dim3(256), 0, s, g_out, ld_gout, D, rowptr, src, N,
                     n_extra, g_h, ld_gh, n_extra > 0 ? g_extra : nullptr);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_gate_blocks_backward(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, float* g_in,
                            int64_t ld_gin, int64_t B, int ns, int nblocks, const int32_t* ls, const int32_t* muls,
                            void* stream) {
  if (B < 0 || ns < 0 || nblocks < 0 || nblocks > 8 || (nblocks > 0 && (!ls || !muls))) return E3_ERR_INVALID_ARG;
  GateBlocksB gb;
  gb.nblocks = nblocks;
  int ngates = 0, wide = 0;
  for (int i = 0; i < 8; ++i) { gb.l[i] = 0; gb.mul[i] = 1 << 30; }
  for (int i = 0; i < nblocks; ++i) {
    if (ls[i] < 0 || ls[i] > 2 || muls[i] < 0) return E3_ERR_INVALID_ARG;
    gb.l[i] = ls[i]; gb.mul[i] = muls[i];
    ngates += muls[i];
    wide += muls[i] * (2 * ls[i] + 1);
  }
  const int W = ns + wide;
  if (ld_in < W + ngates || ld_gout < W || ld_gin < W + ngates) return E3_ERR_INVALID_ARG;
  if (B == 0 || W == 0) return E3_OK;
  if (!in || !g_out || !g_in) return E3_ERR_INVALID_ARG;
  const int64_t total = B * (int64_t)(W + ngates);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(gate_blocks_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, g_out, ld_gout, g_in,
                     ld_gin, B, ns, ngates, W, gb);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_segment_sum_backward(const float* g_agg, int64_t ld_gagg, const int32_t* rowptr, int64_t N, int D, float* g_msg,
                            int64_t ld_gmsg, void* stream) {
  if (N < 0 || D <= 0 || ld_gagg < D || ld_gmsg < D) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!g_agg || !rowptr || !g_msg) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(segment_sum_bwd_kernel, dim3(wave_grid_b(N)), dim3(256), 0, (hipStream_t)stream, g_agg, ld_gagg,
                     rowptr, N, D, g_msg, ld_gmsg);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
