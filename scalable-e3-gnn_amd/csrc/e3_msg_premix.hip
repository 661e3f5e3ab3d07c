// The per-node launches of the SEGNN message function (e3_msg_premix, e3_msg_refresh_rows; include/e3gnn.h).  The dst half
// of TP #1 does not depend on the edge: u_dst = W_dst h_dst is computed once per NODE here (1/24 of the rows) and enters the
// edge kernels as the initial value of the MFMA accumulator.  The same launch leaves, per node, the pre-split fp16 (hi, lo)
// row the weights-stationary kernel gathers (fp32 storage) and the row maximum that bounds the node's messages.
#include "e3_msg_plan.h"
#include "cg_tables.h"

#include <algorithm>
#include <type_traits>

namespace e3 {
#include "e3_tp_mfma_core.h"
#include "e3_msg_common.h"

// ------------------------------------------------------------------------------------------------------------------
// One lane's share of a feature row as B fragments: lane (node j, k group g) reads channels 4 g .. 4 g + 3 and 16 + 4 g ..
// 16 + 4 g + 3 of every 32-channel K step of degree L1, scales them and splits them into (hi, lo).  rowmax joins max |x| of
// what the lane read (FINITE: over the finite values only).  Shared by the pre-mix kernel and msg_refresh_rows_kernel.
// ------------------------------------------------------------------------------------------------------------------
template <int LMAX, int TT, bool IO16, int L1, bool FINITE>
__device__ __forceinline__ void split_degree(const char* row, const int g, const float xs, float& rowmax,
                                             uint4 (&xh)[MsgGeom<LMAX, TT>::KS][2 * L1 + 1],
                                             uint4 (&xl)[MsgGeom<LMAX, TT>::KS][2 * L1 + 1]) {
  using G = MsgGeom<LMAX, TT>;
  constexpr int D1 = 2 * L1 + 1, ES = IO16 ? 2 : 4;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    float x[8][D1];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (16 * (2 * ks + p) < G::H)
        read_piece<D1, IO16>(row + (G::col0(L1) + (32 * ks + 16 * p + 4 * g) * D1) * ES, p, xs, x);
      else
        zero_piece<D1>(p, x);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int aa = 0; aa < D1; ++aa) rowmax = FINITE ? fmax_finite(rowmax, x[i][aa]) : fmaxf(rowmax, fabsf(x[i][aa]));
#pragma unroll
    for (int a = 0; a < D1; ++a) {
      float f[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = x[i][a];
      split8<IO16>(f, xh[ks][a], xl[ks][a]);
    }
  }
}
// the lane's 16-byte units of the node's pre-split row (MsgSplit, e3_msg_common.h): plain stores -- the rows are gathered
// ~24 times through the L2
template <int LMAX, int L1>
__device__ __forceinline__ void store_split_degree(uint4* noderow, const int g, const uint4 (&xh)[2 * L1 + 1],
                                                   const uint4 (&xl)[2 * L1 + 1]) {
#pragma unroll
  for (int a = 0; a < 2 * L1 + 1; ++a) {
    noderow[MsgSplit<LMAX>::unit(L1 * L1 + a, 0, g)] = xh[a];
    noderow[MsgSplit<LMAX>::unit(L1 * L1 + a, 1, g)] = xl[a];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// pre-mix: U[n] = (W_dst * sw) (h[n] * xs) for every path of TP #1, in the layout the edge kernel reads as accumulator
// initial values.  One wave per 16 nodes; inputs straight from global memory (each lane reads its own k slots).
// ------------------------------------------------------------------------------------------------------------------
template <int LMAX, int TT, bool IO16>
__global__ __launch_bounds__(256) void msg_premix_kernel(const void* __restrict__ hv, int64_t ldh, int64_t N,
                                                         const float* __restrict__ packed,
                                                         const float* __restrict__ in_scale, float* __restrict__ U,
                                                         uint4* __restrict__ split, float* __restrict__ hmax) {
  using G = MsgGeom<LMAX, TT>;
  constexpr int ES = IO16 ? 2 : 4;
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float xs = (!IO16 && in_scale) ? in_scale[0] : 1.0f;
  constexpr bool STAGE = G::KS == 1;  // (two K steps: the 6 weight blocks of a scalar path would take 96 registers)
  __shared__ __align__(16) float stage_all[STAGE ? 4 * 16 * (6 * 16 + 4) : 4];
  float* stage = stage_all + (STAGE ? ((threadIdx.x >> 6) * 16 * (6 * 16 + 4)) : 0);
  TpCtx cx;
  cx.w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(packed + G::o_w), 0, 3 * G::nblk() * 2048, 0x00020000);
  cx.wrole = 2 * G::nblk() * 2048;  // role 2
  cx.woff = lane * 16; cx.ud = nullptr; cx.wd = nullptr; cx.dsc = 0.f;
  const int64_t ntiles = (N + 15) / 16;
  for (int64_t tile = wave0; tile < ntiles; tile += nw) {
    const int64_t n = tile * 16 + j;
    const bool ok = n < N;
    const char* row = reinterpret_cast<const char*>(hv) + (ok ? n : N - 1) * ldh * ES;
    float* urow = U + (ok ? n : N - 1) * (int64_t)G::UD + 4 * g;
    float rowmax = 0.f;  // max |h[n] * xs| over this lane's channels (joined over the 4 lanes of the node below)
    auto per_l1 = [&](auto l1tag) {
      constexpr int L1 = decltype(l1tag)::value, D1 = 2 * L1 + 1;
      uint4 xh[G::KS][D1], xl[G::KS][D1];
      split_degree<LMAX, TT, IO16, L1, false>(row, g, xs, rowmax, xh, xl);
      if constexpr (!IO16 && G::KS == 1) {  // the B fragments of the weights-stationary edge kernel: it gathers them as they are
        if (split && ok) store_split_degree<LMAX, L1>(split + n * MsgSplit<LMAX>::UNITS, g, xh[0], xl[0]);
      }
      auto per_path = [&](auto l2tag, auto l3tag) {
        constexpr int L2 = decltype(l2tag)::value, L3 = decltype(l3tag)::value;
        if constexpr (G::ok(L1, L2, L3)) {
          constexpr int T = G::T(L3), B0 = G::blk(L1, L2, L3), U0 = G::uoff(L1, L2, L3);
          if constexpr (STAGE) {
            // Component-outer: the path's T weight blocks stay in registers, each component's [16 nodes][T x 16 channels]
            // block is transposed through LDS and leaves as 16-byte units that are CONTIGUOUS per node row (128 or 384
            // bytes) -- the direct form below stores 64-byte pieces, and the launch runs at the per-CU rate of such stores.
            uint4 wh[T][G::KS], wl[T][G::KS];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
              for (int ks = 0; ks < G::KS; ++ks) load_w<IO16>(cx, B0 + ks * T + t, wh[t][ks], wl[t][ks]);
            constexpr int RSP = T * 16 + 4, UPR = T * 4;  // stage row stride (floats), 16-byte units per row
#pragma unroll
            for (int a = 0; a < D1; ++a) {
#pragma unroll
              for (int t = 0; t < T; ++t) {
                f32x4 u = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < G::KS; ++ks) u = mma3<IO16>(wh[t][ks], wl[t][ks], xh[ks][a], xl[ks][a], u);
                *reinterpret_cast<f32x4*>(stage + j * RSP + t * 16 + 4 * g) = u;
              }
              wave_sync_lds();
#pragma unroll
              for (int it = 0; it < (16 * UPR + 63) / 64; ++it) {
                const int unit = it * 64 + lane, row = unit / UPR, col = unit - row * UPR;
                const int64_t nn = tile * 16 + row;
                if (unit < 16 * UPR && nn < N)
                  *reinterpret_cast<f32x4*>(U + nn * (int64_t)G::UD + U0 + a * T * 16 + col * 4) =
                      *reinterpret_cast<const f32x4*>(stage + row * RSP + col * 4);
              }
              wave_sync_lds();
            }
          } else {
#pragma unroll
            for (int t = 0; t < T; ++t) {
              f32x4 u[D1];
#pragma unroll
              for (int a = 0; a < D1; ++a) u[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int ks = 0; ks < G::KS; ++ks) {
                uint4 ah, al;
                load_w<IO16>(cx, B0 + ks * T + t, ah, al);
#pragma unroll
                for (int a = 0; a < D1; ++a) u[a] = mma3<IO16>(ah, al, xh[ks][a], xl[ks][a], u[a]);
              }
              if (ok) {
#pragma unroll
                for (int a = 0; a < D1; ++a) *reinterpret_cast<f32x4*>(urow + U0 + (a * T + t) * 16) = u[a];
              }
            }
          }
        }
      };
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      using I2 = std::integral_constant<int, 2>;
      per_path(I0{}, I0{}); per_path(I1{}, I0{}); per_path(I2{}, I0{});
      per_path(I0{}, I1{}); per_path(I1{}, I1{}); per_path(I2{}, I1{});
      per_path(I0{}, I2{}); per_path(I1{}, I2{}); per_path(I2{}, I2{});
    };
    per_l1(std::integral_constant<int, 0>{});
    per_l1(std::integral_constant<int, 1>{});
    if constexpr (LMAX == 2) per_l1(std::integral_constant<int, 2>{});
    // per-node row maximum (scaled units): the weights-stationary edge kernel bounds a row's messages with it
    rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 16));
    rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 32));
    if (hmax && ok && lane < 16) hmax[n] = rowmax;
  }
}

// Rows of h that changed after the pre-mix launch (ghost rows after a halo exchange) and are only GATHERED as src rows: their
// pre-split row and row maximum again (the table rows belong to dst nodes and are not touched).  One wave per 16 listed nodes;
// the maxima are over the finite values (the operand-scale contract: a NaN / inf ghost row does not trip the overflow guard).
template <int LMAX, int TT, bool IO16>
__global__ __launch_bounds__(256) void msg_refresh_rows_kernel(const void* __restrict__ hv, int64_t ldh, int64_t N,
                                                               const int64_t* __restrict__ rows, int64_t n_rows,
                                                               const float* __restrict__ in_scale, uint4* __restrict__ split,
                                                               float* __restrict__ hmax) {
  constexpr int ES = IO16 ? 2 : 4;
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int64_t tile = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t idx = tile * 16 + j;
  if (tile * 16 >= n_rows) return;
  const int64_t n = rows[idx < n_rows ? idx : n_rows - 1];
  const bool ok = idx < n_rows && n >= 0 && n < N;
  const float xs = (!IO16 && in_scale) ? in_scale[0] : 1.0f;
  const char* row = reinterpret_cast<const char*>(hv) + (ok ? n : 0) * ldh * ES;
  float rowmax = 0.f;
  auto per_l1 = [&](auto l1tag) {
    constexpr int L1 = decltype(l1tag)::value, D1 = 2 * L1 + 1;
    uint4 xh[MsgGeom<LMAX, TT>::KS][D1], xl[MsgGeom<LMAX, TT>::KS][D1];
    split_degree<LMAX, TT, IO16, L1, true>(row, g, xs, rowmax, xh, xl);
    if constexpr (!IO16 && MsgGeom<LMAX, TT>::KS == 1) {
      if (split && ok) store_split_degree<LMAX, L1>(split + n * MsgSplit<LMAX>::UNITS, g, xh[0], xl[0]);
    }
  };
  per_l1(std::integral_constant<int, 0>{});
  per_l1(std::integral_constant<int, 1>{});
  if constexpr (LMAX == 2) per_l1(std::integral_constant<int, 2>{});
  rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 16));
  rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 32));
  if (ok && lane < 16) hmax[n] = rowmax;
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
// [shape index][0 fp32 / 1 bf16 storage]; bf16 storage for H >= 32 (MsgShape::bf16)
struct NodeKernels { const void *premix[2], *refresh[2]; };
template <int LMAX, int TT>
static NodeKernels node_kernels() {
  NodeKernels k = {{(const void*)msg_premix_kernel<LMAX, TT, false>, nullptr},
                   {(const void*)msg_refresh_rows_kernel<LMAX, TT, false>, nullptr}};
  if constexpr (TT >= 2) {
    k.premix[1] = (const void*)msg_premix_kernel<LMAX, TT, true>;
    k.refresh[1] = (const void*)msg_refresh_rows_kernel<LMAX, TT, true>;
  }
  return k;
}
#define E3_MSG_NODE_ENTRY(I, LMAX, TT) node_kernels<LMAX, TT>(),
static const NodeKernels kNodeKernels[kMsgShapes] = {E3_MSG_SHAPES(E3_MSG_NODE_ENTRY)};
#undef E3_MSG_NODE_ENTRY

// the table row (UD floats) + the pre-split row (plans of the weights-stationary kernel) + one float of the row maxima
static MsgPremixLayout premix_layout(const e3_msg_plan* P, int64_t N) {
  return msg_premix_layout(P->k->UD, msg_ws_split_floats(P->lmax, P->H), N);
}

}  // namespace e3

using namespace e3;

extern "C" {

int64_t e3_msg_premix_floats_per_node(const e3_msg_plan* P) { return P ? premix_layout(P, 0).per_node : -1; }
int e3_msg_premix_regions(const e3_msg_plan* P, int64_t N, int64_t* split_offset, int64_t* split_floats_per_node,
                          int64_t* row_max_offset) {
  if (!P || N < 0) return E3_ERR_INVALID_ARG;
  const MsgPremixLayout L = premix_layout(P, N);
  if (split_offset) *split_offset = L.split;
  if (split_floats_per_node) *split_floats_per_node = msg_ws_split_floats(P->lmax, P->H);
  if (row_max_offset) *row_max_offset = L.hmax;
  return E3_OK;
}
int e3_msg_premix(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const void* packed, const float* in_scale,
                  float* premix, int dtype, void* stream) {
  if (!P || N < 0) return E3_ERR_INVALID_ARG;
  if (!e3_msg_supports(P, dtype)) return E3_ERR_UNSUPPORTED;
  const MsgShape& k = *P->k;
  const int io = dtype == E3_BF16 ? 1 : 0, es = io ? 2 : 4;
  if (N == 0) return E3_OK;
  if (!h || !packed || !premix || ld_h < k.D) return E3_ERR_INVALID_ARG;
  if ((ld_h * es & 15) || ((uintptr_t)h & 15) || ((uintptr_t)premix & 15)) return E3_ERR_INVALID_ARG;  // 16-byte row accesses
  int st = msg_ensure_device(P);
  if (st != E3_OK) return st;
  const int64_t ntiles = (N + 15) / 16;
  const int grid = (int)std::min<int64_t>((ntiles + 3) / 4, 2048);
  const MsgPremixLayout L = premix_layout(P, N);
  float* hmax = premix + L.hmax;
  // the pre-split rows: written for the storage type whose edge kernel gathers them (fp32); the region stays unused otherwise
  uint4* split = (L.hmax > L.split && msg_ws_supported(P->lmax, P->H, dtype) && !io) ? reinterpret_cast<uint4*>(premix + L.split)
                                                                                  : nullptr;
  void* args[] = {&h, &ld_h, &N, &packed, &in_scale, &premix, &split, &hmax};
  if (hipLaunchKernel(kNodeKernels[k.index].premix[io], dim3(grid), dim3(256), args, 0, (hipStream_t)stream) != hipSuccess) return E3_ERR_HIP;
  return E3_OK;
}

int e3_msg_refresh_rows(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const int64_t* rows, int64_t n_rows,
                        const float* in_scale, float* premix, int dtype, void* stream) {
  if (!P || N < 0 || n_rows < 0) return E3_ERR_INVALID_ARG;
  if (!e3_msg_supports(P, dtype)) return E3_ERR_UNSUPPORTED;
  const MsgShape& k = *P->k;
  const int io = dtype == E3_BF16 ? 1 : 0, es = io ? 2 : 4;
  if (N == 0 || n_rows == 0) return E3_OK;
  if (!h || !rows || !premix || ld_h < k.D) return E3_ERR_INVALID_ARG;
  if ((ld_h * es & 15) || ((uintptr_t)h & 15) || ((uintptr_t)premix & 15)) return E3_ERR_INVALID_ARG;
  const int64_t nblocks = ((n_rows + 15) / 16 + 3) / 4;
  if (nblocks > 0x7fffffffLL) return E3_ERR_INVALID_ARG;
  const MsgPremixLayout L = premix_layout(P, N);
  float* hmax = premix + L.hmax;
  uint4* split = (L.hmax > L.split && msg_ws_supported(P->lmax, P->H, dtype) && !io) ? reinterpret_cast<uint4*>(premix + L.split)
                                                                                  : nullptr;
  void* args[] = {&h, &ld_h, &N, &rows, &n_rows, &in_scale, &split, &hmax};
  if (hipLaunchKernel(kNodeKernels[k.index].refresh[io], dim3((int)nblocks), dim3(256), args, 0, (hipStream_t)stream) != hipSuccess)
    return E3_ERR_HIP;
  return E3_OK;
}

}  // extern "C"
