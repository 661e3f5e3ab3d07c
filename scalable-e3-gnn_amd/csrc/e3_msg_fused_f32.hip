// Device code of the message function that has to be compiled in ONE translation unit: the fp32-storage instantiations of
// the one-wave-per-tile kernel (e3_msg_fused_kernel.h; all three periodicity modes) and the weight-packing kernels.
//
// Why together: both msg_fused_kernel<.., false, ..> and msg_pack_kernel<float> derive a power-of-two scale with
// pow2_scale_from_bits (e3_tp_mfma_core.h), with targets 10 and 13.  In a translation unit whose callers all pass the same
// target hipcc specialises that function for it before inlining, and every one of these kernels then compiles to different
// instructions.  The kernels were tuned and measured in the unspecialised form, which they keep only side by side
// (profiles/msg_split_isa.txt).  The bf16-storage instantiations do not call it: e3_msg_fused_bf16.hip.
#include "e3_msg_plan.h"
#include "cg_tables.h"

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

namespace e3 {
#include "e3_tp_mfma_core.h"
#include "e3_msg_common.h"
#include "e3_msg_fused_kernel.h"

const MsgFusedKernels& msg_fused_kernels_f32() {
  static const MsgFusedKernels k = msg_fused_kernels<false>();
  return k;
}

// ------------------------------------------------------------------------------------------------------------------
// weight packing (launched by e3_msg_pack_weights, e3_msg_pack.hip)
// ------------------------------------------------------------------------------------------------------------------
__global__ void msg_absmax_kernel(MsgPackArgs a, uint32_t* hdr) {  // fp32 storage only
  float m1 = 0.f, m2 = 0.f;
  for (int c = 0; c < 3; ++c) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.nw1[c]; i += (int64_t)gridDim.x * blockDim.x)
      m1 = fmax_finite(m1, static_cast<const float*>(a.w1[c])[i]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < a.nw2[c]; i += (int64_t)gridDim.x * blockDim.x)
      m2 = fmax_finite(m2, static_cast<const float*>(a.w2[c])[i]);
  }
  for (int o = 32; o > 0; o >>= 1) { m1 = fmaxf(m1, __shfl_xor(m1, o)); m2 = fmaxf(m2, __shfl_xor(m2, o)); }
  if ((threadIdx.x & 63) == 0) {
    if (m1 > 0.f) atomicMax(hdr + 0, __builtin_bit_cast(uint32_t, m1));
    if (m2 > 0.f) atomicMax(hdr + 3, __builtin_bit_cast(uint32_t, m2));
  }
}

// T = float: fp16 (hi, lo) halves of w * sw.  T = bf16 (bf16 storage): the bf16 weights themselves in the hi half, sw = 1.
template <typename T>
__global__ void msg_pack_kernel(MsgPackArgs a, const MsgPackDesc* desc, int ndesc, float* packed) {
  constexpr bool IO16 = std::is_same<T, bf16>::value;
  const uint32_t* hb = reinterpret_cast<const uint32_t*>(packed);
  const float sw1 = IO16 ? 1.0f : pow2_scale_from_bits(hb[0], 13), sw2 = IO16 ? 1.0f : pow2_scale_from_bits(hb[3], 13);
  auto rd = [](const void* p, int64_t i) { return to_acc(static_cast<const T*>(p)[i]); };
  for (int r = blockIdx.x; r < ndesc; r += gridDim.x) {
    const MsgPackDesc q = desc[r];
    const void* W = q.role == 1 ? a.w2[q.mat] : a.w1[q.mat];
    const float sw = q.role == 1 ? sw2 : sw1;
    uint16_t* dst = reinterpret_cast<uint16_t*>(packed + a.o_w + ((size_t)q.role * a.nblk + q.blk) * 512);
    for (int i = threadIdx.x; i < 512; i += blockDim.x) {
      const int lane = i >> 3, jj = i & 7, ch = lane & 15, g = lane >> 4;
      const int k = kperm(g, jj);
      float v = 0.f;
      if (k < q.nvalid && q.colbase + ch < q.M) v = rd(W, (int64_t)(q.rowbase + k) * q.M + q.colbase + ch) * sw;
      if constexpr (IO16) {
        dst[lane * 8 + jj] = __builtin_bit_cast(uint16_t, (__bf16)v);
        dst[512 + lane * 8 + jj] = 0;
      } else {
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        dst[lane * 8 + jj] = __builtin_bit_cast(uint16_t, hi);
        dst[512 + lane * 8 + jj] = __builtin_bit_cast(uint16_t, lo);
      }
    }
  }
  if (blockIdx.x == 0) {
    // norm tables in accumulator order, already divided by the weight scale; d-term weights scaled like the others
    for (int i = threadIdx.x; i < a.NS * 16; i += blockDim.x) {
      const int s = i >> 4, ch = i & 15;
      const int T0 = a.TT * (1 + a.LMAX);
      int l3, t, c;
      if (s < T0) { l3 = 0; t = s; c = 0; }
      else if (s < T0 + 3 * a.TT) { l3 = 1; t = (s - T0) / 3; c = (s - T0) % 3; }
      else { l3 = 2; t = (s - T0 - 3 * a.TT) / 5; c = (s - T0 - 3 * a.TT) % 5; }
      const int idx = (16 * t + ch) * (2 * l3 + 1) + c;
      packed[a.o_norm1 + i] = (a.n1[l3] ? rd(a.n1[l3], idx) : 1.0f) / sw1;
      packed[a.o_norm2 + i] = (a.n2[l3] ? rd(a.n2[l3], idx) : 1.0f) / sw2;
    }
    for (int i = threadIdx.x; i < a.WD; i += blockDim.x) {
      const int T0 = a.TT * (1 + a.LMAX);
      int l, rem;
      if (i < T0 * 16) { l = 0; rem = i; }
      else if (i < (T0 + a.TT) * 16) { l = 1; rem = i - T0 * 16; }
      else { l = 2; rem = i - (T0 + a.TT) * 16; }
      const int M = l == 0 ? a.M0 : a.H;
      packed[a.o_wd + i] = rd(a.w1[l], (int64_t)a.rowd[l] * M + rem) * sw1;
    }
    if (threadIdx.x == 0) {
      packed[1] = sw1; packed[2] = 1.0f / sw1;
      packed[4] = sw2; packed[5] = 1.0f / sw2;
    }
    // header[6]: Bw with |gated message of product #1| <= Bw * max|input of the row| (true units):
    //   |sum_paths sum_a z[a][c] (W^T x)[a][w]| <= kZMax * (column sum of |W|) * max|x|,   kZMax = max over paths of
    //   max_c sum_a ||C[a][.][c]||_2 * sqrt(2 l2 + 1) = 5 (component-normalised harmonics; oracle/cg.py tables), gates <= 1.
    // The weights-stationary kernel derives the per-row power-of-two scale of product #2's fp16 (hi, lo) operands from it
    // (e3_msg_ws.hip); a bound that is loose by up to 2^14 costs no accuracy there.
    __shared__ uint32_t red[2];
    float bw = 0.f;
    for (int l = 0; l <= a.LMAX; ++l) {
      const int M = l == 0 ? a.M0 : a.H;
      const int rows = (int)(a.nw1[l] / M);
      if (threadIdx.x < 2) red[threadIdx.x] = 0u;
      __syncthreads();
      float cs = 0.f, nm = 0.f;
      for (int col = threadIdx.x; col < M; col += blockDim.x) {
        float sum = 0.f;
        for (int r = 0; r < rows; ++r) sum += fabsf(rd(a.w1[l], (int64_t)r * M + col));
        cs = fmaxf(cs, sum);
      }
      for (int i = threadIdx.x; i < M * (2 * l + 1); i += blockDim.x) nm = fmaxf(nm, a.n1[l] ? fabsf(rd(a.n1[l], i)) : 1.0f);
      if (cs > 0.f && cs < INFINITY) atomicMax(&red[0], __builtin_bit_cast(uint32_t, cs));
      if (nm > 0.f && nm < INFINITY) atomicMax(&red[1], __builtin_bit_cast(uint32_t, nm));
      __syncthreads();
      bw = fmaxf(bw, 5.0f * __builtin_bit_cast(float, red[0]) * __builtin_bit_cast(float, red[1]));
      __syncthreads();
    }
    if (threadIdx.x == 0) packed[6] = bw;
  }
}

int msg_pack_launch(const MsgPackArgs& a, const MsgPackDesc* d_desc, int ndesc, int dtype, void* packed, hipStream_t s) {
  E3_HIP_CHECK(hipMemsetAsync(packed, 0, 256, s));
  const dim3 grid(std::min<int>(ndesc, 512));
  if (dtype == E3_F32) {
    hipLaunchKernelGGL(msg_absmax_kernel, dim3(64), dim3(256), 0, s, a, (uint32_t*)packed);
    hipLaunchKernelGGL(msg_pack_kernel<float>, grid, dim3(256), 0, s, a, d_desc, ndesc, (float*)packed);
  } else {
    hipLaunchKernelGGL(msg_pack_kernel<bf16>, grid, dim3(256), 0, s, a, d_desc, ndesc, (float*)packed);
  }
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // namespace e3

#if E3_MSG_STAMP
extern "C" int e3_msg_debug_stamps(unsigned long long* out8, int reset) {
  if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(e3::g_msg_stamps), 64) != hipSuccess) return E3_ERR_HIP;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(e3::g_msg_stamps), z, 64) != hipSuccess) return E3_ERR_HIP;
  }
  return E3_OK;
}
#endif
