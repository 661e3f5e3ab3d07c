// Fused weight gradient of one output class of the general SH tensor product (fp32; e3_tp_backward_weights):
// grad_W[c3][krow][w] += sum_{b,c} F[b,c,krow] G[b,c,w] with the features F and
// the normalised output gradient G of a row tile built in LDS and contracted on v_mfma_f32_32x32x2_f32 (exact fp32 products) --
// nothing of size [B, D3, K] reaches HBM.  One workgroup = 4 waves; output tiles of 32 x 32 are dealt to the waves round-robin,
// their accumulators live in registers over the whole row range of the workgroup and leave through atomics at the end.
// LDS: x (class order) and y of R rows, Fs [R D3][ldF], Gs [R D3][ldG]; ldF, ldG = 32 (mod 64) floats, so that the two k rows of
// one MFMA operand read (lanes 0-31 / 32-63) fall on different banks.
#include "e3_tp_cg.h"

namespace e3 {

template <typename G>
__device__ __forceinline__ void tp_wgrad_feat_item(const float* x, const float* y, float* F, int ldF) {
  if constexpr (G::ok) {
    float f[G::D3];
    G::feat(x, y, f);
#pragma unroll
    for (int c = 0; c < G::D3; ++c) F[c * ldF] = f[c];
  }
}

typedef float tp_f32x16 __attribute__((ext_vector_type(16)));

// workgroup barrier that orders LDS accesses only: __syncthreads() also waits for every global load in flight (vmcnt(0)), which
// would end the register prefetch of the next row tile at the first barrier after it was issued
__device__ __forceinline__ void tp_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int NTW, int RT>
__global__ __launch_bounds__(256) void tp_wgrad_mfma_kernel(const float* __restrict__ in1, int64_t ld1,
                                                            const float* __restrict__ in2, int64_t ld2,
                                                            const float* __restrict__ packed, const float* __restrict__ go,
                                                            int64_t ldg, float* __restrict__ gw, int c3, int ldF, int ldG,
                                                            int64_t B, TpDev p) {
  using A = float;
  constexpr int R = RT;
  constexpr int XC = 3, GC = 2;   // columns of x / (c, w) pairs of G per thread (host: D1 <= 768, D3 M <= 512, RT Dy <= 256)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int l3 = c3 >> 1, D3 = 2 * l3 + 1, K = p.K[c3], M = p.M[c3];
  float* xs = reinterpret_cast<float*>(smem_raw);
  float* ys = xs + (size_t)R * p.D1;
  float* Fs = ys + (((size_t)R * p.Dy + 3) & ~(size_t)3);
  float* Gs = Fs + (size_t)R * D3 * ldF;
  // the class's path descriptors in LDS (l1, l2, wrow, n, cbase): a GLOBAL read inside the tile loop is followed by vmcnt(0), which
  // would also wait for the whole register prefetch issued just before it
  int* ptab = reinterpret_cast<int*>(Gs + (size_t)R * D3 * ldG);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* normcol = packed + p.normcol_off;
  const int tm = (K + 31) / 32, tn = (M + 31) / 32, ntile = tm * tn;
  const int npath = p.npath[c3];
  if (tid < npath) {
    const TpPath P = p.paths[p.poff[c3] + tid];
    ptab[8 * tid] = P.l1; ptab[8 * tid + 1] = P.l2; ptab[8 * tid + 2] = P.wrow; ptab[8 * tid + 3] = p.n[P.c1]; ptab[8 * tid + 4] = p.cbase[P.c1];
  }
  tp_f32x16 acc[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // padding columns are zero for the whole launch (the row passes never write them)
  for (int i = tid; i < R * D3 * ldF; i += 256) Fs[i] = 0.f;
  for (int i = tid; i < R * D3 * ldG; i += 256) Gs[i] = 0.f;
  // this thread's share of a tile's global reads (fixed for the launch): columns tid + 256 j of x, pairs tid + 256 j of G, one y
  int xcp[XC], gdst[GC], goc[GC];
  float gnv[GC];
  const int per = D3 * M;
#pragma unroll
  for (int j = 0; j < XC; ++j) xcp[j] = tid + 256 * j < p.D1 ? p.cpos[tid + 256 * j] : -1;
#pragma unroll
  for (int j = 0; j < GC; ++j) {
    const int e = tid + 256 * j;
    goc[j] = -1; gdst[j] = 0; gnv[j] = 0.f;
    if (e < per) {
      const int c = e / M, w = e - c * M;
      goc[j] = p.ocol[p.ocol_off[c3] + w] + c;
      gnv[j] = normcol[goc[j]];
      gdst[j] = c * ldG + w;
    }
  }
  const int yr_r = tid / p.Dy, yr_d = tid - yr_r * p.Dy;
  const bool yok = tid < R * p.Dy;
  // The rows of the NEXT tile travel in registers while this tile is contracted: issued right after the LDS image of the current
  // tile is complete, stored at the top of the next iteration (the loads of a tile used to be waited for in place)
  float xr[XC][RT], gr[GC][RT], yr = 0.f;
  auto issue = [&](const int64_t row0) {
    if (row0 + RT <= B) {   // whole tile inside the batch (every tile but the last): no per-row predicate, i.e. no branch per load
#pragma unroll
      for (int j = 0; j < XC; ++j)
        if (xcp[j] >= 0) {
#pragma unroll
          for (int u = 0; u < RT; ++u) xr[j][u] = in1[(row0 + u) * ld1 + tid + 256 * j];
        }
#pragma unroll
      for (int j = 0; j < GC; ++j)
        if (goc[j] >= 0) {
#pragma unroll
          for (int u = 0; u < RT; ++u) gr[j][u] = go[(row0 + u) * ldg + goc[j]];
        }
      if (yok) yr = in2[(row0 + yr_r) * ld2 + yr_d];
      return;
    }
#pragma unroll
    for (int j = 0; j < XC; ++j)
      if (xcp[j] >= 0) {
#pragma unroll
        for (int u = 0; u < RT; ++u) xr[j][u] = row0 + u < B ? in1[(row0 + u) * ld1 + tid + 256 * j] : 0.f;
      }
#pragma unroll
    for (int j = 0; j < GC; ++j)
      if (goc[j] >= 0) {
#pragma unroll
        for (int u = 0; u < RT; ++u) gr[j][u] = row0 + u < B ? go[(row0 + u) * ldg + goc[j]] : 0.f;
      }
    if (yok) yr = row0 + yr_r < B ? in2[(row0 + yr_r) * ld2 + yr_d] : 0.f;
  };
  const int64_t ntiles = (B + R - 1) / R;
  if ((int64_t)blockIdx.x < ntiles) issue((int64_t)blockIdx.x * R);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform trip count per block: barriers are safe
    tp_lds_barrier();   // the previous tile's features / MFMA operands have been read
#pragma unroll
    for (int j = 0; j < XC; ++j)
      if (xcp[j] >= 0) {
#pragma unroll
        for (int u = 0; u < RT; ++u) xs[u * p.D1 + xcp[j]] = xr[j][u];
      }
#pragma unroll
    for (int j = 0; j < GC; ++j)
      if (goc[j] >= 0) {
#pragma unroll
        for (int u = 0; u < RT; ++u) Gs[(size_t)u * D3 * ldG + gdst[j]] = gr[j][u] * gnv[j];
      }
    if (yok) ys[tid] = yr;
    tp_lds_barrier();
    if (tile + gridDim.x < ntiles) issue((tile + gridDim.x) * R);
    // features of the tile: wave w owns rows w R/4 .. (w + 1) R/4; a path with n channels puts 64 / np2(n) rows side by side in
    // the 64 lanes (rows past B: x = y = 0 -> zero features)
    {
      const int rw = R >> 2, rbase = wave * rw;
      for (int pi = 0; pi < npath; ++pi) {
        const int Pl1 = __builtin_amdgcn_readfirstlane(ptab[8 * pi]), Pl2 = __builtin_amdgcn_readfirstlane(ptab[8 * pi + 1]);
        const int Pwrow = __builtin_amdgcn_readfirstlane(ptab[8 * pi + 2]), n = __builtin_amdgcn_readfirstlane(ptab[8 * pi + 3]);
        const int Pcb = __builtin_amdgcn_readfirstlane(ptab[8 * pi + 4]);
        int sh = 6;                                   // np2 = 1 << sh >= n, at most 64
        while (sh > 0 && (1 << (sh - 1)) >= n) --sh;
        const int np2 = 1 << sh, rpi = 64 >> sh, sub = lane >> sh, k0 = lane & (np2 - 1);
        for (int rb = 0; rb < rw; rb += rpi) {
          const int r = rbase + rb + sub;
          for (int k = k0; k < n; k += np2) {   // (one trip unless n > 64)
            if (rb + sub < rw) {
              E3_TP_PATH_SWITCH(Pl1, Pl2, l3, (tp_wgrad_feat_item<G>(xs + r * p.D1 + Pcb + k * G::D1,
                                                                     ys + r * p.Dy + G::D2 / 2 * (G::D2 / 2),
                                                                     Fs + (size_t)r * G::D3 * ldF + Pwrow + k, ldF)))
            }
          }
        }
      }
    }
    tp_lds_barrier();
    const int kh = lane >> 5, i32 = lane & 31;
    const int nk = R * D3;  // k rows of this tile (even: R is a multiple of 2)
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int tt = wave + 4 * t;
      if (tt < ntile) {
        const int mi = tt / tn, ni = tt - mi * tn;
        const float* fa = Fs + kh * ldF + 32 * mi + i32;
        const float* gb = Gs + kh * ldG + 32 * ni + i32;
        tp_f32x16 a = acc[t];
        for (int kk = 0; kk < nk; kk += 2) a = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk * ldF], gb[kk * ldG], a, 0, 0, 0);
        acc[t] = a;
      }
    }
  }
  // accumulators -> grad_W (C layout of the 32 x 32 MFMA: register r of lane l = C[8 (r >> 2) + 4 (l >> 5) + (r & 3)][l & 31])
#pragma unroll
  for (int t = 0; t < NTW; ++t) {
    const int tt = wave + 4 * t;
    if (tt < ntile) {
      const int mi = tt / tn, ni = tt - mi * tn;
      const int w = 32 * ni + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int krow = 32 * mi + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (krow < K && w < M) atomicAdd(&gw[(size_t)krow * M + w], acc[t][r]);
      }
    }
  }
}

static int tp_wgrad_geometry(const TpDev& p, int c3, int* R, int* ldF, int* ldG, size_t* lds, int* ntw) {
  const int D3 = 2 * (c3 >> 1) + 1, K = p.K[c3], M = p.M[c3];
  if (K <= 0 || M <= 0) return E3_ERR_INVALID_ARG;
  auto pad = [](int v) { int q = (v + 31) / 32 * 32; return (q % 64 == 32) ? q : q + 32; };
  *ldF = pad(K);
  *ldG = pad(M);
  const int ntile = ((K + 31) / 32) * ((M + 31) / 32);
  *ntw = (ntile + 3) / 4;
  if (*ntw > 8) return E3_ERR_UNSUPPORTED;
  auto need_of = [&](int r) {
    return ((size_t)r * p.D1 + (((size_t)r * p.Dy + 3) & ~(size_t)3) + (size_t)r * D3 * (*ldF + *ldG)) * sizeof(float) + 64 * 8 * sizeof(int);
  };
  // per-thread register share of a tile's reads (tp_wgrad_mfma_kernel): 3 columns of x, 2 (c, w) pairs of G, one y
  if (p.D1 > 768 || D3 * M > 512 || p.npath[c3] > 64) return E3_ERR_UNSUPPORTED;
  for (int r : {16, 8})
    if (need_of(r) <= (size_t)76 * 1024 && r * p.Dy <= 256) { *R = r; *lds = need_of(r); return E3_OK; }
  if (need_of(8) <= (size_t)150 * 1024) { *R = 8; *lds = need_of(8); return E3_OK; }
  return E3_ERR_UNSUPPORTED;
}

}  // namespace e3

using namespace e3;

extern "C" int e3_tp_backward_weights(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                                      const void* packed, const void* grad_out, int64_t ldg, void* const grad_weights[6],
                                      int64_t B, int dtype, void* stream) {
  if (!plan || B < 0 || !grad_weights) return E3_ERR_INVALID_ARG;
  if (dtype != E3_F32) return E3_ERR_UNSUPPORTED;
  if (B == 0) return E3_OK;
  if (!in1 || !in2 || !packed || !grad_out) return E3_ERR_INVALID_ARG;
  if (!tp_rows_ok(plan->dev, ld1, ld2, true, ldg)) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  const TpDev& p = plan->dev;
  // every requested class must have a kernel before anything is launched (the caller falls back as a whole)
  int R[6], ldF[6], ldG[6], ntw[6];
  size_t lds[6];
  for (int c = 0; c < 6; ++c) {
    if (!grad_weights[c]) continue;
    st = tp_wgrad_geometry(p, c, &R[c], &ldF[c], &ldG[c], &lds[c], &ntw[c]);
    if (st != E3_OK) return st;
  }
  // [(ntw + 1) / 2 - 1][R == 16]: output tiles per wave rounded up to 2, 4, 6, 8; 8 or 16 rows per tile
  static constexpr decltype(&tp_wgrad_mfma_kernel<2, 8>) kernels[4][2] = {
      {tp_wgrad_mfma_kernel<2, 8>, tp_wgrad_mfma_kernel<2, 16>}, {tp_wgrad_mfma_kernel<4, 8>, tp_wgrad_mfma_kernel<4, 16>},
      {tp_wgrad_mfma_kernel<6, 8>, tp_wgrad_mfma_kernel<6, 16>}, {tp_wgrad_mfma_kernel<8, 8>, tp_wgrad_mfma_kernel<8, 16>}};
  for (int c = 0; c < 6; ++c) {
    if (!grad_weights[c]) continue;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(156 * 1024) / lds[c]));
    st = tp_launch(kernels[(ntw[c] + 1) / 2 - 1][R[c] == 16], R[c], 256 * per_cu, lds[c], B, (hipStream_t)stream, in1, ld1, in2,
                   ld2, packed, grad_out, ldg, grad_weights[c], c, ldF[c], ldG[c], B, p);
    if (st != E3_OK) return st;
  }
  return E3_OK;
}
