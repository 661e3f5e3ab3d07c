// Backward of the edge / node stages around the tensor product (forward: e3_edge_ops.hip) -- what parameter gradients and
// forces through a whole SEGNN layer need besides the tensor product's own backward (e3_l1tp_backward / e3_tp_backward) and
// the derivatives of the edge geometry (e3_edge_geometry_bwd.hip).  Builder-defined stages; the
// reference's contract for its operator is plain torch autograd (l1_tensor_prod.py:234-299), and these kernels are that
// for the stages it does not contain.  fp32, one wave per CSR row where a row is reduced, HBM-bound streaming kernels.
#include "e3_common.h"

namespace e3 {

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

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }

// out = [silu(s) | sigmoid(g_k) v_k]:  d silu = sig (1 + s (1 - sig));  g_v = sig(g) gout;  g_g = sig (1 - sig) sum_m v gout
// One thread per INPUT column (scalar, gate or gated component): the gate column sums over its channel's components.
__global__ __launch_bounds__(256) void gate_blocks_bwd_kernel(const float* __restrict__ in, int64_t ld_in,
                                                              const float* __restrict__ gout, int64_t ld_go,
                                                              float* __restrict__ gin, int64_t ld_gi, int64_t B, int ns,
                                                              int ngates, int W, GateBlocks gb) {
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
                                                               int ngates, int W, GateBlocks gb) {
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

}  // namespace e3

using namespace e3;

extern "C" {

int e3_gate_blocks_backward2(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, const float* c,
                             int64_t ld_c, float* cot_g_out, int64_t ld_cgout, float* cot_in, int64_t ld_cin, int64_t B,
                             int ns, int nblocks, const int32_t* ls, const int32_t* muls, void* stream) {
  GateBlocks gb;
  int ngates, W;
  if (B < 0 || make_gate_blocks(ns, nblocks, ls, muls, &gb, &ngates, &W) != E3_OK) return E3_ERR_INVALID_ARG;
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

int e3_gather_concat_backward(const float* g_out, int64_t ld_gout, int D, const int32_t* rowptr, const int32_t* src,
                              int64_t N, int n_extra, float* g_h, int64_t ld_gh, float* g_extra, void* stream) {
  if (N < 0 || D <= 0 || n_extra < 0 || n_extra > 64 || ld_gout < 2 * D + n_extra || ld_gh < D) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!g_out || !rowptr || !src || !g_h) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  E3_HIP_CHECK(hipMemset2DAsync(g_h, (size_t)ld_gh * 4, 0, (size_t)D * 4, (size_t)N, s));
  hipLaunchKernelGGL(gather_concat_bwd_kernel, dim3(wave_grid(N)), dim3(256), 0, s, g_out, ld_gout, D, rowptr, src, N,
                     n_extra, g_h, ld_gh, n_extra > 0 ? g_extra : nullptr);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_gate_blocks_backward(const float* in, int64_t ld_in, const float* g_out, int64_t ld_gout, float* g_in,
                            int64_t ld_gin, int64_t B, int ns, int nblocks, const int32_t* ls, const int32_t* muls,
                            void* stream) {
  GateBlocks gb;
  int ngates, W;
  if (B < 0 || make_gate_blocks(ns, nblocks, ls, muls, &gb, &ngates, &W) != E3_OK) return E3_ERR_INVALID_ARG;
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
  hipLaunchKernelGGL(segment_sum_bwd_kernel, dim3(wave_grid(N)), dim3(256), 0, (hipStream_t)stream, g_agg, ld_gagg,
                     rowptr, N, D, g_msg, ld_gmsg);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
