// Backward of the general SH tensor product on generic FMA kernels (fp32 / fp64; the reference's operator gets its gradients
// from torch autograd over l1_tensor_prod.py:240-299 -- these kernels are that for l <= 2): the rows / weights kernels behind
// e3_tp_backward, and the operands / contract passes around library GEMMs behind e3_tp_backward_operands / _contract.
// The fp32-MFMA weight gradient is e3_tp_wgrad.hip.
#include "e3_tp_cg.h"

namespace e3 {

template <typename T, int R>
__global__ __launch_bounds__(256) void tp_bwd_rows_kernel(const T* __restrict__ in1, int64_t ld1, const T* __restrict__ in2,
                                                          int64_t ld2, const typename AccOf<T>::type* __restrict__ packed,
                                                          const T* __restrict__ go, int64_t ldg, T* __restrict__ gin1,
                                                          int64_t ldg1, typename AccOf<T>::type* __restrict__ gin2,
                                                          int64_t ldg2, int64_t B, TpDev p) {
  using A = typename AccOf<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  A* xs = reinterpret_cast<A*>(smem_raw);
  A* ys = xs + (size_t)R * p.D1;
  A* gs = ys + (size_t)R * p.Dy;
  A* gx = gs + (size_t)R * p.Dout;
  A* gy = gx + (size_t)R * p.D1;
  const int tid = threadIdx.x;
  int Ktot = 0, Mtot = 0;
  for (int c = 0; c < 6; ++c) { Ktot += p.n[c]; Mtot += p.M[c]; }
  const A* normcol = packed + p.normcol_off;
  const int64_t ntiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    tp_stage_rows<T, A>(in1, ld1, in2, ld2, go, ldg, normcol, row0, R, B, p, xs, ys, gs);
    for (int i = tid; i < R * 9; i += 256) gy[i] = 0;
    __syncthreads();
    if (gin1) {  // thread = (row, in channel): sum over every path that reads this channel and every out channel
      for (int i = tid; i < R * Ktot; i += 256) {
        int r = i / Ktot, kk = i - r * Ktot, c1 = 0;
        while (kk >= p.n[c1]) { kk -= p.n[c1]; ++c1; }
        const int l1 = c1 >> 1, D1c = 2 * l1 + 1;
        A acc[5] = {0, 0, 0, 0, 0};
        const A* y = ys + r * p.Dy;
        for (int c3 = 0; c3 < 6; ++c3) {
          const int l3 = c3 >> 1, M = p.M[c3];
          for (int pi = 0; pi < p.npath[c3]; ++pi) {
            const TpPath P = p.paths[p.poff[c3] + pi];
            if (P.c1 != c1) continue;
            const A* W = packed + p.woff[c3] + (int64_t)(P.wrow + kk) * M;
            const A* yl = y + P.l2 * P.l2;
            for (int w = 0; w < M; ++w) {
              const A* g = gs + r * p.Dout + p.ocol[p.ocol_off[c3] + w];
              const A wv = W[w];
              E3_TP_PATH_SWITCH(l1, P.l2, l3, G::gx(wv, yl, g, acc))
            }
          }
        }
        for (int a = 0; a < D1c; ++a) gx[r * p.D1 + p.cbase[c1] + kk * D1c + a] = acc[a];
      }
    }
    if (gin2) {  // thread = (row, out channel): partial sums over the in channels, reduced through LDS atomics
      for (int i = tid; i < R * Mtot; i += 256) {
        int r = i / Mtot, w = i - r * Mtot, c3 = 0;
        while (w >= p.M[c3]) { w -= p.M[c3]; ++c3; }
        const int l3 = c3 >> 1, M = p.M[c3];
        const A* g = gs + r * p.Dout + p.ocol[p.ocol_off[c3] + w];
        A loc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int pi = 0; pi < p.npath[c3]; ++pi) {
          const TpPath P = p.paths[p.poff[c3] + pi];
          const int D1c = 2 * P.l1 + 1;
          const A* xc = xs + r * p.D1 + p.cbase[P.c1];
          const A* W = packed + p.woff[c3] + (int64_t)P.wrow * M + w;
          for (int k = 0; k < p.n[P.c1]; ++k) {
            const A wv = W[(int64_t)k * M];
            E3_TP_PATH_SWITCH(P.l1, P.l2, l3, G::gy(wv, xc + k * D1c, g, loc + P.l2 * P.l2))
          }
        }
        for (int q = 0; q < p.Dy; ++q) atomicAdd(&gy[r * 9 + q], loc[q]);
      }
    }
    __syncthreads();
    if (gin1)
      for (int i = tid; i < R * p.D1; i += 256) {
        int r = i / p.D1, d = i - r * p.D1;
        if (row0 + r < B) gin1[(row0 + r) * ldg1 + d] = from_acc<T, A>(gx[r * p.D1 + p.cpos[d]]);
      }
    if (gin2)
      for (int i = tid; i < R * p.Dy; i += 256) {
        int r = i / p.Dy, q = i - r * p.Dy;
        if (row0 + r < B) {
          if (ldg2 == 0) atomicAdd(&gin2[q], gy[r * 9 + q]);   // broadcast in2: one row of sums (caller zero-fills)
          else gin2[(row0 + r) * ldg2 + q] = gy[r * 9 + q];
        }
      }
    __syncthreads();
  }
}

// grad_W[c3][krow][w] += sum_b sum C x y g'   (atomics into zero-filled fp32 / fp64 arrays, one per out class)
template <typename T, int R>
__global__ __launch_bounds__(256) void tp_bwd_w_kernel(const T* __restrict__ in1, int64_t ld1, const T* __restrict__ in2,
                                                       int64_t ld2, const typename AccOf<T>::type* __restrict__ packed,
                                                       const T* __restrict__ go, int64_t ldg,
                                                       typename AccOf<T>::type* g0, typename AccOf<T>::type* g1,
                                                       typename AccOf<T>::type* g2, typename AccOf<T>::type* g3,
                                                       typename AccOf<T>::type* g4, typename AccOf<T>::type* g5,
                                                       int64_t B, TpDev p) {
  using A = typename AccOf<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  A* xs = reinterpret_cast<A*>(smem_raw);
  A* ys = xs + (size_t)R * p.D1;
  A* gs = ys + (size_t)R * p.Dy;
  A* gw[6] = {g0, g1, g2, g3, g4, g5};
  const int tid = threadIdx.x;
  const A* normcol = packed + p.normcol_off;
  int64_t Wtot = 0;
  for (int c = 0; c < 6; ++c) Wtot += (int64_t)p.K[c] * p.M[c];
  const int64_t ntiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    __syncthreads();
    tp_stage_rows<T, A>(in1, ld1, in2, ld2, go, ldg, normcol, row0, R, B, p, xs, ys, gs);
    __syncthreads();
    for (int64_t i = tid; i < Wtot; i += 256) {
      int64_t e = i;
      int c3 = 0;
      while (e >= (int64_t)p.K[c3] * p.M[c3]) { e -= (int64_t)p.K[c3] * p.M[c3]; ++c3; }
      if (!gw[c3]) continue;
      const int M = p.M[c3], krow = (int)(e / M), w = (int)(e - (int64_t)krow * M), l3 = c3 >> 1;
      TpPath P = p.paths[p.poff[c3]];
      for (int pi = 0; pi < p.npath[c3]; ++pi) {
        const TpPath Q = p.paths[p.poff[c3] + pi];
        if (krow >= Q.wrow) P = Q;
      }
      const int kk = krow - P.wrow, D1c = 2 * P.l1 + 1;
      const int oc = p.ocol[p.ocol_off[c3] + w];
      A acc = 0;
      for (int r = 0; r < R; ++r) {
        const A* x = xs + r * p.D1 + p.cbase[P.c1] + kk * D1c;
        const A* y = ys + r * p.Dy + P.l2 * P.l2;
        const A* g = gs + r * p.Dout + oc;
        E3_TP_PATH_SWITCH(P.l1, P.l2, l3, acc += G::gw(x, y, g))
      }
      atomicAdd(&gw[c3][e], acc);
    }
  }
}

template <typename T>
static int tp_launch_bwd(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                         const void* packed, const void* go, int64_t ldg, void* gin1, int64_t ldg1, void* gin2,
                         int64_t ldg2, void* const gw[6], int64_t B, hipStream_t s) {
  using A = typename AccOf<T>::type;
  const TpDev& p = plan->dev;
  if (gin1 || gin2) {
    constexpr int R = 4;
    const size_t lds = (size_t)R * (2 * p.D1 + p.Dy + p.Dout + 9) * sizeof(A);
    const int st = tp_launch(tp_bwd_rows_kernel<T, R>, R, 256 * 4, lds, B, s, in1, ld1, in2, ld2, packed, go, ldg, gin1, ldg1,
                             gin2, ldg2, B, p);
    if (st != E3_OK) return st;
  }
  bool anyw = false;
  for (int c = 0; gw && c < 6; ++c) anyw |= gw[c] != nullptr;
  if (!anyw) return E3_OK;
  constexpr int RW = 8;
  const size_t lds = (size_t)RW * (p.D1 + p.Dy + p.Dout) * sizeof(A);
  return tp_launch(tp_bwd_w_kernel<T, RW>, RW, 256 * 2, lds, B, s, in1, ld1, in2, ld2, packed, go, ldg, gw[0], gw[1], gw[2],
                   gw[3], gw[4], gw[5], B, p);
}


// ---------------------------------------------------------------------------------------------------
// Backward as two thin passes around library GEMMs (the large-B path; the kernels above stay as the small-B / reference
// path).  Per output class c3 (D3 = 2 l3 + 1, K = weight rows, M = weight cols):
//   operands:  F[b, c, krow] = sum_{a,bq} C[a][bq][c] x[b,k,a] y[b,bq]      G[b, c, w] = grad_out[b, (w,c)] * norm[w,c]
//   caller:    grad_W = F^T G   (one GEMM over the B * D3 rows)             T = G W^T  (same shape as F)
//   contract:  grad_in1[b,k,a] = sum_paths sum_{bq,c} C y[b,bq] T[b,c,wrow+k]   grad_in2[b,bq] = sum_paths sum_{k,a,c} C x T
// One wave owns one row; lanes run over the channels k of a path, so F / T accesses are contiguous runs.
// ---------------------------------------------------------------------------------------------------
// one path, RW rows of one wave: features of channel k = lane, lane + 64, ... (everything indexed at compile time)
template <typename G, typename A, int RW>
__device__ __forceinline__ void tp_bwd_feat_path(const A* xb, int ldx, const A* yb, int ldy, int n, int lane, int nrow,
                                                 A* F, int K) {
  if constexpr (G::ok) {
    for (int k = lane; k < n; k += 64) {
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        if (q < nrow) {
          A f[G::D3];
          G::feat(xb + q * ldx + k * G::D1, yb + q * ldy + G::D2 / 2 * (G::D2 / 2), f);
          A* Fr = F + (int64_t)q * G::D3 * K + k;
#pragma unroll
          for (int c = 0; c < G::D3; ++c) Fr[(int64_t)c * K] = f[c];
        }
      }
    }
  }
}

template <typename G, typename A, int RW>
__device__ __forceinline__ void tp_bwd_contract_path(const A* xb, A* gxb, int ldx, const A* yb, int ldy, int n, int lane,
                                                     const A* ts, int K, A (&gy)[RW][9]) {
  if constexpr (G::ok) {
    constexpr int L2 = G::D2 / 2;
    for (int k = lane; k < n; k += 64) {
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        A t[G::D3], ga[G::D1], gq[G::D2];
#pragma unroll
        for (int c = 0; c < G::D3; ++c) t[c] = ts[(q * G::D3 + c) * K + k];
#pragma unroll
        for (int a = 0; a < G::D1; ++a) ga[a] = 0;
#pragma unroll
        for (int j = 0; j < G::D2; ++j) gq[j] = 0;
        G::gxy(xb + q * ldx + k * G::D1, yb + q * ldy + L2 * L2, t, ga, gq);
        A* gc = gxb + q * ldx + k * G::D1;
#pragma unroll
        for (int a = 0; a < G::D1; ++a) gc[a] += ga[a];
#pragma unroll
        for (int j = 0; j < G::D2; ++j) gy[q][L2 * L2 + j] += gq[j];
      }
    }
  }
}

// RW rows per wave (4 waves, R = 4 RW rows per block): the RW rows of a wave go through every path together, so their
// loads / stores are in flight at the same time
template <typename T, int RW>
__global__ __launch_bounds__(256) void tp_bwd_operands_kernel(const T* __restrict__ in1, int64_t ld1,
                                                              const T* __restrict__ in2, int64_t ld2,
                                                              const typename AccOf<T>::type* __restrict__ packed,
                                                              const T* __restrict__ go, int64_t ldg, TpPtr6 Fp, TpPtr6 Gp,
                                                              int64_t B, TpDev p) {
  using A = typename AccOf<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  constexpr int R = 4 * RW;
  A* xs = reinterpret_cast<A*>(smem_raw);
  A* ys = xs + (size_t)R * p.D1;
  A* gs = ys + (size_t)R * p.Dy;  // grad_out * norm, original column order (staged with x and y: one round of loads per tile)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const A* normcol = packed + p.normcol_off;
  const int64_t ntiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform trip count per block: barriers are safe
    const int64_t row0 = tile * R;
    __syncthreads();
    tp_stage_rows<T, A>(in1, ld1, in2, ld2, go, ldg, normcol, row0, R, B, p, xs, ys, gs);
    __syncthreads();
    const int64_t wrow0 = row0 + wave * RW;
    for (int c3 = 0; c3 < 6; ++c3) {
      const int l3 = c3 >> 1, D3 = 2 * l3 + 1, M = p.M[c3], K = p.K[c3];
      if (M == 0 || K == 0) continue;
      A* F = static_cast<A*>(Fp.p[c3]);
      A* Gm = static_cast<A*>(Gp.p[c3]);
      if (F) {
        for (int pi = 0; pi < p.npath[c3]; ++pi) {
          const TpPath P = p.paths[p.poff[c3] + pi];
          const int n = p.n[P.c1];
          const A* xb = xs + wave * RW * p.D1 + p.cbase[P.c1];
          const A* yb = ys + wave * RW * p.Dy;
          const int nrow = B - wrow0 < RW ? (int)(B - wrow0) : RW;  // <= 0 for a wave past the end
          E3_TP_PATH_SWITCH(P.l1, P.l2, l3, (tp_bwd_feat_path<G, A, RW>(xb, p.D1, yb, p.Dy, n, lane, nrow,
                                                                        F + wrow0 * G::D3 * (int64_t)K + P.wrow, K)))
        }
      }
      if (Gm) {
        for (int i = lane; i < D3 * M; i += 64) {
          const int c = i / M, w = i - c * M;
          const int oc = p.ocol[p.ocol_off[c3] + w] + c;
#pragma unroll
          for (int q = 0; q < RW; ++q)
            if (wrow0 + q < B) Gm[(wrow0 + q) * D3 * (int64_t)M + i] = gs[(wave * RW + q) * p.Dout + oc];
        }
      }
    }
  }
}

template <typename T, int RW>
__global__ __launch_bounds__(256) void tp_bwd_contract_kernel(const T* __restrict__ in1, int64_t ld1,
                                                              const T* __restrict__ in2, int64_t ld2, TpPtr6 Tp,
                                                              T* __restrict__ gin1, int64_t ldg1,
                                                              typename AccOf<T>::type* __restrict__ gin2, int64_t ldg2,
                                                              int64_t B, TpDev p) {
  using A = typename AccOf<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  constexpr int R = 4 * RW;
  A* xs = reinterpret_cast<A*>(smem_raw);
  A* ys = xs + (size_t)R * p.D1;
  A* gx = ys + (size_t)R * p.Dy;
  A* ts = gx + (size_t)R * p.D1;  // the R rows of T, class after class: [c3][row][c][K] (a flat copy of each class's rows)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t ntiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    const int nr = B - row0 < R ? (int)(B - row0) : R;
    __syncthreads();
    {  // every load of the tile is issued here, back to back; the path loop below only touches LDS
      A* td = ts;
      for (int c3 = 0; c3 < 6; ++c3) {
        const A* Tm = static_cast<const A*>(Tp.p[c3]);
        const int per = (2 * (c3 >> 1) + 1) * p.K[c3];
        if (!Tm || per == 0 || p.M[c3] == 0) continue;
        const A* src = Tm + row0 * per;
        for (int i = tid; i < nr * per; i += 256) td[i] = src[i];
        td += R * per;
      }
    }
    tp_stage_rows<T, A>(in1, ld1, in2, ld2, nullptr, 0, nullptr, row0, R, B, p, xs, ys, nullptr);
    for (int i = tid; i < R * p.D1; i += 256) gx[i] = 0;
    __syncthreads();
    const int64_t wrow0 = row0 + wave * RW;
    A gy[RW][9];
#pragma unroll
    for (int q = 0; q < RW; ++q)
#pragma unroll
      for (int j = 0; j < 9; ++j) gy[q][j] = 0;
    const A* tc = ts;
    for (int c3 = 0; c3 < 6; ++c3) {
      const int l3 = c3 >> 1, D3 = 2 * l3 + 1, K = p.K[c3];
      if (!Tp.p[c3] || K == 0 || p.M[c3] == 0) continue;
      for (int pi = 0; pi < p.npath[c3]; ++pi) {
        const TpPath P = p.paths[p.poff[c3] + pi];
        // lane <-> channel is the same for every path of a class: no race on gx.  Rows past B hold stale LDS: their
        // results stay in LDS / registers and are dropped
        E3_TP_PATH_SWITCH(P.l1, P.l2, l3, (tp_bwd_contract_path<G, A, RW>(
                                              xs + wave * RW * p.D1 + p.cbase[P.c1], gx + wave * RW * p.D1 + p.cbase[P.c1],
                                              p.D1, ys + wave * RW * p.Dy, p.Dy, p.n[P.c1], lane,
                                              tc + wave * RW * G::D3 * K + P.wrow, K, gy)))
      }
      tc += R * D3 * K;
    }
    if (gin2) {
#pragma unroll
      for (int q = 0; q < RW; ++q) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          A v = gy[q][j];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
          gy[q][j] = v;
        }
        if (wrow0 + q < B && lane < p.Dy) {
          A v = gy[q][0];
#pragma unroll
          for (int j = 1; j < 9; ++j) v = lane == j ? gy[q][j] : v;
          if (ldg2 == 0) atomicAdd(&gin2[lane], v);
          else gin2[(wrow0 + q) * ldg2 + lane] = v;
        }
      }
    }
    __syncthreads();
    if (gin1)
      for (int i = tid; i < nr * p.D1; i += 256) {
        int r = i / p.D1, d = i - r * p.D1;
        gin1[(row0 + r) * ldg1 + d] = from_acc<T, A>(gx[r * p.D1 + p.cpos[d]]);
      }
  }
}

template <typename T>
static int tp_launch_bwd_operands(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                                  const void* packed, const void* go, int64_t ldg, void* const F[6], void* const G[6],
                                  int64_t B, hipStream_t s) {
  using A = typename AccOf<T>::type;
  const TpDev& p = plan->dev;
  TpPtr6 f, g;
  for (int c = 0; c < 6; ++c) { f.p[c] = F ? F[c] : nullptr; g.p[c] = G ? G[c] : nullptr; }
  constexpr int RW = 2, R = 4 * RW;
  const size_t lds = (size_t)R * (p.D1 + p.Dy + p.Dout) * sizeof(A);
  return tp_launch(tp_bwd_operands_kernel<T, RW>, R, 256 * 8, lds, B, s, in1, ld1, in2, ld2, packed, go, ldg, f, g, B, p);
}

template <typename A>
static size_t tp_bwd_contract_lds(const TpDev& p, int R) {
  size_t trow = 0;
  for (int c = 0; c < 6; ++c)
    if (p.M[c] > 0) trow += (size_t)(2 * (c >> 1) + 1) * p.K[c];
  return (size_t)R * (2 * p.D1 + p.Dy + trow) * sizeof(A);
}

template <typename T>
static int tp_launch_bwd_contract(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                                  void* const Tm[6], void* gin1, int64_t ldg1, void* gin2, int64_t ldg2, int64_t B,
                                  hipStream_t s) {
  using A = typename AccOf<T>::type;
  const TpDev& p = plan->dev;
  TpPtr6 t;
  for (int c = 0; c < 6; ++c) t.p[c] = (p.M[c] > 0 && p.K[c] > 0) ? Tm[c] : nullptr;
  for (int c = 0; c < 6; ++c)
    if (p.M[c] > 0 && p.K[c] > 0 && !Tm[c]) return E3_ERR_INVALID_ARG;  // every class with weights has a T
  // rows per block by LDS budget: 4 blocks per CU (40 KB each) if possible
  if (tp_bwd_contract_lds<A>(p, 8) <= 40 * 1024)
    return tp_launch(tp_bwd_contract_kernel<T, 2>, 8, 256 * 8, tp_bwd_contract_lds<A>(p, 8), B, s, in1, ld1, in2, ld2, t, gin1,
                     ldg1, gin2, ldg2, B, p);
  return tp_launch(tp_bwd_contract_kernel<T, 1>, 4, 256 * 8, tp_bwd_contract_lds<A>(p, 4), B, s, in1, ld1, in2, ld2, t, gin1,
                   ldg1, gin2, ldg2, B, p);
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_tp_backward(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                   const void* packed, const void* grad_out, int64_t ldg, void* grad_in1, int64_t ldg1,
                   void* grad_in2, int64_t ldg2, void* const grad_weights[6], int64_t B, int dtype, void* stream) {
  if (!plan || B < 0 || (dtype != E3_F32 && dtype != E3_F64)) return E3_ERR_INVALID_ARG;
  if (B == 0) return E3_OK;
  if (!in1 || !in2 || !packed || !grad_out) return E3_ERR_INVALID_ARG;
  if (!tp_rows_ok(plan->dev, ld1, ld2, true, ldg)) return E3_ERR_INVALID_ARG;
  if (!tp_grad_rows_ok(plan->dev, grad_in1, ldg1, grad_in2, ldg2, ld2)) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  return tp_by_dtype(dtype, [&](auto tag) {
    return tp_launch_bwd<typename decltype(tag)::type>(plan, in1, ld1, in2, ld2, packed, grad_out, ldg, grad_in1, ldg1,
                                                       grad_in2, ldg2, grad_weights, B, (hipStream_t)stream);
  });
}

int e3_tp_backward_operands(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                            const void* packed, const void* grad_out, int64_t ldg, void* const features[6],
                            void* const gout[6], int64_t B, int dtype, void* stream) {
  if (!plan || B < 0 || (dtype != E3_F32 && dtype != E3_F64)) return E3_ERR_INVALID_ARG;
  if (B == 0) return E3_OK;
  if (!in1 || !in2 || !packed || (!features && !gout) || (gout && !grad_out)) return E3_ERR_INVALID_ARG;
  if (!tp_rows_ok(plan->dev, ld1, ld2, gout != nullptr, ldg)) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  return tp_by_dtype(dtype, [&](auto tag) {
    return tp_launch_bwd_operands<typename decltype(tag)::type>(plan, in1, ld1, in2, ld2, packed, grad_out, ldg, features,
                                                                gout, B, (hipStream_t)stream);
  });
}

int e3_tp_backward_contract(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                            void* const t[6], void* grad_in1, int64_t ldg1, void* grad_in2, int64_t ldg2, int64_t B,
                            int dtype, void* stream) {
  if (!plan || B < 0 || (dtype != E3_F32 && dtype != E3_F64)) return E3_ERR_INVALID_ARG;
  if (B == 0) return E3_OK;
  if (!in1 || !in2 || !t || (!grad_in1 && !grad_in2)) return E3_ERR_INVALID_ARG;
  if (!tp_rows_ok(plan->dev, ld1, ld2, false, 0)) return E3_ERR_INVALID_ARG;
  if (!tp_grad_rows_ok(plan->dev, grad_in1, ldg1, grad_in2, ldg2, ld2)) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  return tp_by_dtype(dtype, [&](auto tag) {
    return tp_launch_bwd_contract<typename decltype(tag)::type>(plan, in1, ld1, in2, ld2, t, grad_in1, ldg1, grad_in2, ldg2,
                                                                B, (hipStream_t)stream);
  });
}

}  // extern "C"
