// L1 tensor product: the device loops its generic kernels share (e3_l1tp.hip, e3_l1tp_bwd.hip; the norm expansion also
// e3_l1tp_mfma.hip).  Every sum runs over its index upwards, one multiply-add per term: the callers' results are pinned bit
// for bit (tests/test_l1tp_parent_bits_gpu.py), so the order of the terms is part of these functions' contract.
#pragma once
#include "e3_l1tp_plan.h"

namespace e3 {

template <typename A> struct L1Vec3 { A x, y, z; };

// W-mixes of ONE output channel of class cls from a staged canonical in1 row x: t0 = sum_k s[k] W[k] over the scalar block,
// a = sum_k v[k] W[ns + k] over the slot-1 vectors, b the same over the cross block (zero for a scalar class, which has
// none).  W points at the channel's column of the class's matrix (row stride M), read in the type TW it is stored in
template <typename A> struct L1Mix { A t0; L1Vec3<A> a, b; };
template <typename A, typename TW>
__device__ __forceinline__ L1Vec3<A> l1_mix3(const A* v, const TW* W, const int n, const int M) {
  A ax = 0, ay = 0, az = 0;
  for (int k = 0; k < n; ++k) {
    A wk = to_acc(W[(int64_t)k * M]);
    ax += v[3 * k + 0] * wk;
    ay += v[3 * k + 1] * wk;
    az += v[3 * k + 2] * wk;
  }
  return {ax, ay, az};
}
template <typename A, typename TW>
__device__ __forceinline__ L1Mix<A> l1_mix(const PlanDev& p, const int cls, const A* x, const TW* W, const int M) {
  const int sc = kL1Src[cls][0], va = kL1Src[cls][1];
  const A* s = x + p.cbase[sc];
  const int ns = p.n[sc], na = p.n[va];
  L1Mix<A> m;
  m.t0 = 0;
  for (int k = 0; k < ns; ++k) m.t0 += s[k] * to_acc(W[(int64_t)k * M]);
  const TW* Wa = W + (int64_t)ns * M;
  m.a = l1_mix3<A>(x + p.cbase[va], Wa, na, M);
  m.b = {0, 0, 0};
  if (cls >= 2) {
    const int vb = kL1Src[cls][2];
    m.b = l1_mix3<A>(x + p.cbase[vb], Wa + (int64_t)na * M, p.n[vb], M);
  }
  return m;
}

// weight row `row` of a class's matrix w [rows][M] (NULL: the class has none, the result is zero) against the scalar part
// gg[m], resp. the xyz-interleaved part gg[3 m + c], of a staged grad_out * norm row
template <typename A, typename T>
__device__ __forceinline__ A l1_wdot1(const T* w, const int row, const int M, const A* gg) {
  A acc = 0;
  if (w) {
    const T* W = w + (int64_t)row * M;
    for (int m = 0; m < M; ++m) acc += to_acc(W[m]) * gg[m];
  }
  return acc;
}
template <typename A, typename T>
__device__ __forceinline__ L1Vec3<A> l1_wdot3(const T* w, const int row, const int M, const A* gg) {
  A vx = 0, vy = 0, vz = 0;
  if (w) {
    const T* W = w + (int64_t)row * M;
    for (int m = 0; m < M; ++m) {
      A wk = to_acc(W[m]);
      vx += wk * gg[3 * m];
      vy += wk * gg[3 * m + 1];
      vz += wk * gg[3 * m + 2];
    }
  }
  return {vx, vy, vz};
}

// normcol[out column] = the norm of that column, for every column of the plan (NULL class norm: 1); entry i of class c's norm
// vector belongs to channel i / width, component i % width (L1TP.py:174,178,183,187).  Work item `tid` of `stride`
template <typename T, typename A>
__device__ __forceinline__ void l1_normcol_fill(const PlanDev& p, const L1Ptr4<const T>& nrm, A* normcol, const int64_t tid,
                                                const int64_t stride) {
  for (int c = 0; c < 4; ++c) {
    const int width = (c >= 2) ? 3 : 1;
    for (int64_t i = tid; i < (int64_t)p.M[c] * width; i += stride) {
      int m = (int)(i / width), comp = (int)(i - (int64_t)m * width);
      normcol[p.ocol[p.ocol_off[c] + m] + comp] = nrm.p[c] ? to_acc(nrm.p[c][i]) : A(1);
    }
  }
}

}  // namespace e3
