// General SH tensor product, device side shared by the generic kernels (e3_tp.hip, e3_tp_bwd.hip, e3_tp_wgrad.hip): the
// contractions of one path (l1, l2, l3) over the CG<> table, the one switch from a runtime path to its instantiation, and the
// one row staging.
//   out[b, w, c] = norm[w,c] * sum_paths sum_k W[k, w] * sum_{a,bq} C[a][bq][c] x[b,k,a] y[b,bq]
#pragma once
#include "cg_tables.h"
#include "e3_tp_plan.h"

namespace e3 {

// The loop nests below fix the rounding of out and grad_in1 (a / bq / c order): they are not to be reordered or merged.
template <int L1, int L2, int L3, typename A>
struct TpGrad {
  static constexpr bool ok = CG<L1, L2, L3>::valid;
  static constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
  // forward: o[c] += sum_{a,bq} C T[a] y[bq] with T[a] = sum_k W[k, w] x[k, a] (the channel index contracted first)
  static __device__ __forceinline__ void fwd(const A* __restrict__ x, int n, const A* __restrict__ W, int M,
                                             const A* __restrict__ y, A (&o)[5]) {
    if constexpr (ok) {
      A T[D1];
#pragma unroll
      for (int a = 0; a < D1; ++a) T[a] = 0;
      for (int k = 0; k < n; ++k) {
        const A wk = W[(int64_t)k * M];
#pragma unroll
        for (int a = 0; a < D1; ++a) T[a] += x[k * D1 + a] * wk;
      }
#pragma unroll
      for (int a = 0; a < D1; ++a)
#pragma unroll
        for (int b = 0; b < D2; ++b)
#pragma unroll
          for (int c = 0; c < D3; ++c)
            if (CG<L1, L2, L3>::v[a][b][c] != 0.0) o[c] += A(CG<L1, L2, L3>::v[a][b][c]) * T[a] * y[b];
    }
  }
  // gx[a] += wv * sum_{bq,c} C y[bq] g[c]
  static __device__ __forceinline__ void gx(A wv, const A* y, const A* g, A* gxa) {
    if constexpr (ok) {
#pragma unroll
      for (int a = 0; a < D1; ++a) {
        A s = 0;
#pragma unroll
        for (int bq = 0; bq < D2; ++bq)
#pragma unroll
          for (int c = 0; c < D3; ++c)
            if (CG<L1, L2, L3>::v[a][bq][c] != 0.0) s += A(CG<L1, L2, L3>::v[a][bq][c]) * y[bq] * g[c];
        gxa[a] += wv * s;
      }
    }
  }
  // gy[bq] += wv * sum_{a,c} C x[a] g[c]
  static __device__ __forceinline__ void gy(A wv, const A* x, const A* g, A* gyb) {
    if constexpr (ok) {
#pragma unroll
      for (int bq = 0; bq < D2; ++bq) {
        A s = 0;
#pragma unroll
        for (int a = 0; a < D1; ++a)
#pragma unroll
          for (int c = 0; c < D3; ++c)
            if (CG<L1, L2, L3>::v[a][bq][c] != 0.0) s += A(CG<L1, L2, L3>::v[a][bq][c]) * x[a] * g[c];
        gyb[bq] += wv * s;
      }
    }
  }
  // f[c] = sum_{a,bq} C x[a] y[bq]   (the feature the weight row of channel k multiplies)
  static __device__ __forceinline__ void feat(const A* x, const A* y, A* f) {
    if constexpr (ok) {
#pragma unroll
      for (int c = 0; c < D3; ++c) {
        A s = 0;
#pragma unroll
        for (int a = 0; a < D1; ++a)
#pragma unroll
          for (int bq = 0; bq < D2; ++bq)
            if (CG<L1, L2, L3>::v[a][bq][c] != 0.0) s += A(CG<L1, L2, L3>::v[a][bq][c]) * x[a] * y[bq];
        f[c] = s;
      }
    }
  }
  // from t[c] = sum_w W[k,w] g'[w,c]:  gx[a] += sum_{bq,c} C y[bq] t[c],  gy[bq] += sum_{a,c} C x[a] t[c]
  static __device__ __forceinline__ void gxy(const A* x, const A* y, const A* t, A* gxa, A* gyb) {
    if constexpr (ok) {
#pragma unroll
      for (int a = 0; a < D1; ++a)
#pragma unroll
        for (int bq = 0; bq < D2; ++bq) {
          A s = 0;
#pragma unroll
          for (int c = 0; c < D3; ++c)
            if (CG<L1, L2, L3>::v[a][bq][c] != 0.0) s += A(CG<L1, L2, L3>::v[a][bq][c]) * t[c];
          gxa[a] += s * y[bq];
          gyb[bq] += s * x[a];
        }
    }
  }
  // sum_{a,bq,c} C x[a] y[bq] g[c]
  static __device__ __forceinline__ A gw(const A* x, const A* y, const A* g) {
    A s = 0;
    if constexpr (ok) {
#pragma unroll
      for (int a = 0; a < D1; ++a)
#pragma unroll
        for (int bq = 0; bq < D2; ++bq)
#pragma unroll
          for (int c = 0; c < D3; ++c)
            if (CG<L1, L2, L3>::v[a][bq][c] != 0.0) s += A(CG<L1, L2, L3>::v[a][bq][c]) * x[a] * y[bq] * g[c];
    }
    return s;
  }
};

// The path switch: runs CALL with G = TpGrad<l1, l2, l3, A> for the fifteen couplings of l <= 2 (A is the caller's accumulate
// type); anything else does nothing.
#define E3_TP_PATH_SWITCH(l1, l2, l3, CALL)                                                                  \
  switch ((l1) * 9 + (l2) * 3 + (l3)) {                                                                      \
    case 0: { using G = TpGrad<0, 0, 0, A>; CALL; } break;   case 4: { using G = TpGrad<0, 1, 1, A>; CALL; } break;  \
    case 8: { using G = TpGrad<0, 2, 2, A>; CALL; } break;   case 10: { using G = TpGrad<1, 0, 1, A>; CALL; } break; \
    case 12: { using G = TpGrad<1, 1, 0, A>; CALL; } break;  case 13: { using G = TpGrad<1, 1, 1, A>; CALL; } break; \
    case 14: { using G = TpGrad<1, 1, 2, A>; CALL; } break;  case 16: { using G = TpGrad<1, 2, 1, A>; CALL; } break; \
    case 17: { using G = TpGrad<1, 2, 2, A>; CALL; } break;  case 20: { using G = TpGrad<2, 0, 2, A>; CALL; } break; \
    case 22: { using G = TpGrad<2, 1, 1, A>; CALL; } break;  case 23: { using G = TpGrad<2, 1, 2, A>; CALL; } break; \
    case 24: { using G = TpGrad<2, 2, 0, A>; CALL; } break;  case 25: { using G = TpGrad<2, 2, 1, A>; CALL; } break; \
    case 26: { using G = TpGrad<2, 2, 2, A>; CALL; } break;  default: break;                                    \
  }

// Stage the R rows from row0 of a block into LDS: x through cpos into class order, y, and -- unless go is null -- g' =
// grad_out * norm in the original out column order.  Rows past B read as zero.
template <typename T, typename A>
__device__ __forceinline__ void tp_stage_rows(const T* in1, int64_t ld1, const T* in2, int64_t ld2,
                                              const T* go /*null: no gradient rows*/, int64_t ldg, const A* normcol,
                                              int64_t row0, int R, int64_t B, const TpDev& p, A* xs, A* ys, A* gs) {
  const int tid = threadIdx.x;
  for (int i = tid; i < R * p.D1; i += kTpThreads) {
    int r = i / p.D1, d = i - r * p.D1;
    int64_t row = row0 + r;
    xs[r * p.D1 + p.cpos[d]] = row < B ? to_acc(in1[row * ld1 + d]) : A(0);
  }
  for (int i = tid; i < R * p.Dy; i += kTpThreads) {
    int r = i / p.Dy, d = i - r * p.Dy;
    int64_t row = row0 + r;
    ys[i] = row < B ? to_acc(in2[row * ld2 + d]) : A(0);
  }
  if (!go) return;
  for (int i = tid; i < R * p.Dout; i += kTpThreads) {
    int r = i / p.Dout, d = i - r * p.Dout;
    int64_t row = row0 + r;
    gs[i] = row < B ? to_acc(go[row * ldg + d]) * normcol[d] : A(0);
  }
}

}  // namespace e3
