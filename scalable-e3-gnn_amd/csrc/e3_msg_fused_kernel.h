// The SEGNN message function as ONE launch per layer (BASELINE.json north_star: "fused per-edge CDNA4 HIP kernel"):
//
//     a_i = sum_{e: dst(e) = i}  gate( TP2( gate( TP1( [h_dst | h_src | d_e] ; Y_e ) ) ; Y_e ) )
//
// per 16-edge tile and wave: spherical harmonics from the two positions, message TP #1, gate, message TP #2, gate and the
// segment-sum over dst -- the [E, 288] messages, Y [E, 9] and d [E] never exist in HBM.  Hidden irreps Hx0e+Hx1o(+Hx2e),
// H in {16, 32, 64}; TP semantics, weight row order and norms are those of e3_tp_* (include/e3gnn.h), i.e. of the
// reference operator for l <= 1 (l1_tensor_prod.py:242-297).
//
// Formulation ("mix first"): for a path (l1, l2, l3) with weights W and coupling z[a][c] = sum_b C[a][b][c] Y_l2[b],
//     out[c][w] = sum_a z[a][c] * u[a][w],      u[a][w] = sum_k W[k][w] x[k][a]
// u is a plain GEMM of the RAW input channels -- the MFMA B operand is x itself, split into fp16 (hi, lo) ONCE per input
// degree and shared by every path and tile -- and the Y-dependent part is a small per-lane fold of accumulator tiles.
// Two consequences used here:
//   * the dst half of TP #1 does not depend on the edge at all: u_dst = W_dst h_dst is computed once per NODE by
//     msg_premix_kernel (1/24 of the rows) and enters the edge kernel as the initial value of the MFMA accumulator;
//   * the gated output of TP #1 sits in accumulator layout (lane = (edge, 4 channels)), which is exactly the B-operand
//     layout of TP #2 when the k order of the weights is permuted to match (kperm below): no transpose between them.
// Paths into scalar outputs (l3 = 0, l1 > 0) are cheaper "feature first": f[k] = sum_a z[a] x[k][a], one MFMA group.
//
// MFMA: v_mfma_f32_16x16x32_f16, A = weights [16 out channels][32 k], B = features [32 k][16 edges], D = [channel 4g + r]
// [edge j] in lane (j = lane & 15, g = lane >> 4).  fp32 products as hi*hi + hi*lo + lo*hi (split2_f16), operands scaled
// by powers of two: weights at pack time (header), h by `in_scale`, the gated messages per edge row in-kernel.
//
// This header is the kernel template; e3_msg_fused_f32.hip and e3_msg_fused_bf16.hip instantiate it for one storage type
// each (18 and 12 of the 30 instantiations) and e3_msg_fused.hip launches them.  Internal header, included inside namespace
// e3 after e3_msg_common.h; the including file has <cstddef>, <type_traits> and <utility>.
#pragma once

#ifndef E3_MSG_STAMP
#define E3_MSG_STAMP 0  // 1: per-phase cycle counters (s_memtime) summed into g_msg_stamps -- development builds only, of the
#endif                  //    fp32 instantiations (tools/build_variant.sh stamp -DE3_MSG_STAMP=1 e3_msg_fused_f32;
                        //    STAMPS=1 tools/msg_micro.py prints them)
#if E3_MSG_STAMP
__device__ unsigned long long g_msg_stamps[8];
#endif

constexpr int kMsgWD = 1;   // weight prefetch distance in blocks (2: 27.1 vs 26.0 ms at 2 waves per SIMD -- registers)
constexpr int kMsgUDP = 1;  // pre-mix prefetch distance in blocks
constexpr int kMsgWPS = 2;  // waves per SIMD the H = 32, l_max = 2 kernel is compiled for (1: 48-55 ms at any prefetch distance)

// ---- one tensor product as a flat, software-pipelined list of blocks ----------------------------------------------
// A block = one 16-channel output tile of one path: its weight operand(s) and (product #1) its 4 D1 pre-mix values are
// fetched while the PREVIOUS block computes, so no block starts with an exposed L2 round trip.  Blocks are ordered by input
// degree; the first block of a degree also loads that degree's inputs, builds the feature-first operand and the (hi, lo)
// halves.  Everything is indexed at compile time (BlkList::at(IDX)); state that survives a block lives in TpState.
struct BlkDesc {
  int l1, l2, l3, t;
  bool ff;             // feature-first path (scalar outputs from l1 > 0)
  bool first_of_l1;    // load / split the inputs of degree l1 here
  bool first_of_path;  // build z here
};
template <int LMAX, int TT>
struct BlkList {
  using G = MsgGeom<LMAX, TT>;
  // order inside a degree: the feature-first path (needs the fp32 inputs), then the mix-first paths by (l3, l2)
  static constexpr BlkDesc at(int idx) {
    int n = 0;
    for (int l1 = 0; l1 <= LMAX; ++l1) {
      bool first = true;
      for (int pass = 0; pass < 2; ++pass)
        for (int l3 = 0; l3 <= LMAX; ++l3)
          for (int l2 = 0; l2 <= LMAX; ++l2) {
            if (!G::ok(l1, l2, l3)) continue;
            const bool ff = l3 == 0 && l1 > 0;
            if (ff != (pass == 0)) continue;
            for (int t = 0; t < G::T(l3); ++t) {
              if (n == idx) return BlkDesc{l1, l2, l3, t, ff, first, t == 0};
              first = false;
              ++n;
            }
          }
    }
    return BlkDesc{-1, 0, 0, 0, false, false, false};
  }
  static constexpr int count() {
    int n = 0;
    while (at(n).l1 >= 0) ++n;
    return n;
  }
};

template <int KS>
struct TpState {
  uint4 xh[KS][5], xl[KS][5];  // (hi, lo) halves of the current degree's inputs, per component
  uint4 fh[KS], fl[KS];        // feature-first operand of the current degree
  float z[5][5];               // coupling of the current path
  // operand rings (all indices are compile-time): block IDX reads slot IDX % (D + 1) and requests block IDX + D
  uint4 wh[kMsgWD + 1][KS], wl[kMsgWD + 1][KS];
  f32x4 uin[kMsgUDP + 1][5];
};

// weights of block IDX and, for product #1, its pre-mix values, both requested one block ahead.  (Measured on 1 M
// particles: a weight prefetch distance of two blocks costs 8 registers -> spills -> 27.1 vs 26.0 ms; touching the
// pre-mix rows of the tile's dst nodes ahead of product #1 (L2 warm-up) 25.9 vs 26.2 ms: neither is kept.)
template <int LMAX, int TT, bool IO16, int IDX>
__device__ __forceinline__ void tp_prefetch_w(const TpCtx& cx, uint4 (&wh)[MsgGeom<LMAX, TT>::KS],
                                              uint4 (&wl)[MsgGeom<LMAX, TT>::KS]) {
  using G = MsgGeom<LMAX, TT>;
  if constexpr (IDX < BlkList<LMAX, TT>::count()) {
    constexpr BlkDesc B = BlkList<LMAX, TT>::at(IDX);
    constexpr int T = G::T(B.l3), B0 = G::blk(B.l1, B.l2, B.l3);
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) load_w<IO16>(cx, B0 + ks * T + B.t, wh[ks], wl[ks]);
  }
}
template <int LMAX, int TT, bool FIRST, int IDX>
__device__ __forceinline__ void tp_prefetch_u(const TpCtx& cx, f32x4 (&uin)[5]) {
  using G = MsgGeom<LMAX, TT>;
  if constexpr (FIRST && IDX < BlkList<LMAX, TT>::count()) {
    constexpr BlkDesc B = BlkList<LMAX, TT>::at(IDX);
    constexpr int T = G::T(B.l3), U0 = G::uoff(B.l1, B.l2, B.l3);
#pragma unroll
    for (int a = 0; a < 2 * B.l1 + 1; ++a) uin[a] = *reinterpret_cast<const f32x4*>(cx.ud + U0 + (a * T + B.t) * 16);
  }
}

template <int LMAX, int TT, bool FIRST, bool IO16, int IDX, class XLOAD>
__device__ __forceinline__ void tp_block(const TpCtx& cx, const float (&y)[9], XLOAD& xload,
                                         TpState<MsgGeom<LMAX, TT>::KS>& st, f32x4 (&acc0)[MsgGeom<LMAX, TT>::T(0)],
                                         f32x4 (&acc1)[TT][3], f32x4 (&acc2)[LMAX == 2 ? TT : 1][5]) {
  using G = MsgGeom<LMAX, TT>;
  using BL = BlkList<LMAX, TT>;
  constexpr int KS = G::KS;
  constexpr BlkDesc B = BL::at(IDX);
  constexpr int L1 = B.l1, L2 = B.l2, L3 = B.l3, t = B.t;
  constexpr int D1 = 2 * L1 + 1, D3 = 2 * L3 + 1;
  // ---- later blocks' operands are requested first ----
  tp_prefetch_w<LMAX, TT, IO16, IDX + kMsgWD>(cx, st.wh[(IDX + kMsgWD) % (kMsgWD + 1)], st.wl[(IDX + kMsgWD) % (kMsgWD + 1)]);
  tp_prefetch_u<LMAX, TT, FIRST, IDX + kMsgUDP>(cx, st.uin[(IDX + kMsgUDP) % (kMsgUDP + 1)]);
  const uint4 (&wh)[KS] = st.wh[IDX % (kMsgWD + 1)];
  const uint4 (&wl)[KS] = st.wl[IDX % (kMsgWD + 1)];
  const f32x4 (&uin)[5] = st.uin[IDX % (kMsgUDP + 1)];
  // ---- first block of a degree: inputs, feature-first operand, (hi, lo) halves ----
  if constexpr (B.first_of_l1) {
    float x[KS][8][D1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xload(std::integral_constant<int, L1>{}, ks, x[ks]);
    if constexpr (L1 > 0 && G::ok(L1, L1, 0)) {
      float zz[D1][1];
      make_z<L1, L1, 0>(y, zz);
#pragma unroll
      for (int a = 0; a < D1; ++a) st.z[a][0] = zz[a][0];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float sum = zz[0][0] * x[ks][i][0];
#pragma unroll
          for (int a = 1; a < D1; ++a) sum = __builtin_fmaf(zz[a][0], x[ks][i][a], sum);
          f[i] = sum;
        }
        split8<IO16>(f, st.fh[ks], st.fl[ks]);
      }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int a = 0; a < D1; ++a) {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = x[ks][i][a];
        split8<IO16>(f, st.xh[ks][a], st.xl[ks][a]);
      }
  }
  if constexpr (B.first_of_path && !B.ff) {
    float zz[D1][D3];
    make_z<L1, L2, L3>(y, zz);
#pragma unroll
    for (int a = 0; a < D1; ++a)
#pragma unroll
      for (int c = 0; c < D3; ++c) st.z[a][c] = zz[a][c];
  }
  // ---- compute ----
  if constexpr (B.ff) {
    f32x4 o = acc0[t];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) o = mma3<IO16>(wh[ks], wl[ks], st.fh[ks], st.fl[ks], o);
    if constexpr (FIRST) {  // dst half: fold of the per-node pre-mix
#pragma unroll
      for (int a = 0; a < D1; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = __builtin_fmaf(uin[a][r], st.z[a][0], o[r]);
    }
    acc0[t] = o;
  } else {
    f32x4 u[D1];
#pragma unroll
    for (int a = 0; a < D1; ++a) {
      if constexpr (FIRST) u[a] = uin[a];
      else u[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (FIRST && L1 == 0) {
      const f32x4 wdv = *reinterpret_cast<const f32x4*>(cx.wd + G::wdoff(L3) + t * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) u[0][r] = __builtin_fmaf(wdv[r], cx.dsc, u[0][r]);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int a = 0; a < D1; ++a) u[a] = mma3<IO16>(wh[ks], wl[ks], st.xh[ks][a], st.xl[ks][a], u[a]);
#pragma unroll
    for (int c = 0; c < D3; ++c)
#pragma unroll
      for (int a = 0; a < D1; ++a)
        if (z_nonzero<L1, L2, L3>(a, c)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (L3 == 0) acc0[t][r] = __builtin_fmaf(u[a][r], st.z[a][c], acc0[t][r]);
            else if constexpr (L3 == 1) acc1[t][c][r] = __builtin_fmaf(u[a][r], st.z[a][c], acc1[t][c][r]);
            else acc2[t][c][r] = __builtin_fmaf(u[a][r], st.z[a][c], acc2[t][c][r]);
          }
        }
  }
  if constexpr (IDX + 1 < BL::count())
    tp_block<LMAX, TT, FIRST, IO16, IDX + 1>(cx, y, xload, st, acc0, acc1, acc2);
}

// One tensor product on the lane's 16-edge tile.  XLOAD(l1tag, ks, x[8][D1]) delivers the (scaled) fp32 inputs of this
// lane: x[jj][a] = channel 32 ks + kperm(g, jj), component a.  acc0 / acc1 / acc2: output tiles per degree.
template <int LMAX, int TT, bool FIRST, bool IO16, class XLOAD>
__device__ __forceinline__ void tp_core(const TpCtx& cx, const float (&y)[9], XLOAD&& xload,
                                        f32x4 (&acc0)[MsgGeom<LMAX, TT>::T(0)], f32x4 (&acc1)[TT][3],
                                        f32x4 (&acc2)[LMAX == 2 ? TT : 1][5]) {
  constexpr int KS = MsgGeom<LMAX, TT>::KS;
  TpState<KS> st;
  // prologue of the rings: blocks 0 .. D - 1
  auto prime = [&](auto itag) {
    constexpr int I = decltype(itag)::value;
    if constexpr (I < kMsgWD) tp_prefetch_w<LMAX, TT, IO16, I>(cx, st.wh[I % (kMsgWD + 1)], st.wl[I % (kMsgWD + 1)]);
    if constexpr (I < kMsgUDP) tp_prefetch_u<LMAX, TT, FIRST, I>(cx, st.uin[I % (kMsgUDP + 1)]);
  };
  prime(std::integral_constant<int, 0>{}); prime(std::integral_constant<int, 1>{});
  prime(std::integral_constant<int, 2>{}); prime(std::integral_constant<int, 3>{});
  static_assert(kMsgWD <= 4 && kMsgUDP <= 4, "ring prologue");
  tp_block<LMAX, TT, FIRST, IO16, 0>(cx, y, xload, st, acc0, acc1, acc2);
}
// ------------------------------------------------------------------------------------------------------------------
// the edge kernel
// ------------------------------------------------------------------------------------------------------------------
constexpr int msg_waves_per_simd(int lmax, int tt) {
  return (lmax == 2 ? 44 : 20) * tt <= 96 ? ((lmax == 2 && tt == 2) ? kMsgWPS : 2) : 1;
}

// The explicit arguments of msg_fused_kernel as the kernel-argument segment lays them out (in order, natural alignment):
// where the cell instantiations find their cell.  CONTRACT: this is the kernel's parameter list, field for field; the
// static_asserts behind the kernel compare the two and pin the offset, so a parameter added or moved there fails the build
// here instead of reading something else as the cell.
struct MsgFusedKernarg {
  const void* hv; int64_t ldh; const float4* pos4; const int32_t *src, *dst; int64_t E; const float *packed, *U, *in_scale;
  float* out; int64_t ldo; int blk;
  PbcCell cell;
};
template <int LMAX, int TT, bool IO16, int PBC>
// (waves per SIMD fixed from both sides: with the minimum alone the scheduler of a small instantiation -- l_max = 1 needs ~120
// registers -- trades its load / compute overlap for an occupancy the launch does not use: 6.7 -> 8.7 ms)
__global__ __launch_bounds__(256, msg_waves_per_simd(LMAX, TT))
__attribute__((amdgpu_waves_per_eu(msg_waves_per_simd(LMAX, TT), msg_waves_per_simd(LMAX, TT)))) void msg_fused_kernel(
    const void* __restrict__ hv, int64_t ldh, const float4* __restrict__ pos4, const int32_t* __restrict__ src,
    const int32_t* __restrict__ dst, int64_t E, const float* __restrict__ packed, const float* __restrict__ U,
    const float* __restrict__ in_scale, float* __restrict__ out, int64_t ldo, int blk,
    const typename PbcArg<PBC>::type box) {
  using G = MsgGeom<LMAX, TT>;
  constexpr int H = G::H, D = G::D, T0 = G::T(0), NS = G::NS;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (j = lane & 15 = the lane's edge, g = lane >> 4 = its channel group: every phase of the tile loop derives them from a
  // regenerated lane id, see item "nothing waits behind the atomics" in DESIGN.md §4.1)

  // workgroup tables: norm1 (x 1/xs), norm2, d-term weights
  float* n1tab = lds;
  float* n2tab = n1tab + NS * 16;
  float* wdtab = n2tab + NS * 16;
  float* wbuf = wdtab + G::WD + (size_t)wave * G::lds_wave;
  int* idbuf = reinterpret_cast<int*>(wdtab + G::WD + (size_t)4 * G::lds_wave) + wave * 64;  // edge ids of the wave's next tile
  // bf16 storage needs no operand scales (bf16 has the fp32 exponent range): xs = 1, messages unscaled
  constexpr int ES = IO16 ? 2 : 4;  // bytes per stored feature element
  const char* h = reinterpret_cast<const char*>(hv);
  const float xs = (!IO16 && in_scale) ? in_scale[0] : 1.0f, ixs = (!IO16 && in_scale) ? in_scale[1] : 1.0f;
  for (int i = tid; i < NS * 16; i += blockDim.x) {
    n1tab[i] = packed[G::o_norm1 + i] * ixs;
    n2tab[i] = packed[G::o_norm2 + i];
  }
  for (int i = tid; i < G::WD; i += blockDim.x) wdtab[i] = packed[G::o_wd + i];
  __syncthreads();

  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(packed + G::o_w), 0, 3 * G::nblk() * 2048, 0x00020000);

  // tile -> wave map, XCD-aware.  Workgroups b, b + 8, b + 16, ... share an XCD (round-robin dispatch; `b & 7` is a label
  // of the group, not the XCD's id): the group gets one contiguous eighth of the (Morton-ordered) tiles, and INSIDE the
  // eighth its workgroups are dealt chunks of 4 blk tiles round-robin -- so the ~256 waves that share one 4 MiB L2 sweep
  // through the same spatial neighbourhood together and the gathered h[src] / pre-mix rows are fetched once per XCD
  // instead of once per edge.  A wave owns `blk` consecutive tiles of a chunk (its segment sum carries across them).
  // (all of it in 32-bit scalars -- E < 2^31 because the edge ids are int32: 64-bit products are VALU instructions, which
  // turn the tile loop's control flow into vector code with its counters spilled to scratch)
  const int ntiles = (int)((E + 15) / 16);
  const int per_xcd = (int)(gridDim.x >> 3);  // grid is a multiple of 8
  const int tiles_per_xcd = (ntiles + 7) / 8;
  const int xcd_lo = (int)(blockIdx.x & 7) * tiles_per_xcd;
  const int xcd_hi = xcd_lo + tiles_per_xcd < ntiles ? xcd_lo + tiles_per_xcd : ntiles;
  const int wg_idx = (int)(blockIdx.x >> 3);
  const int Ei = (int)E;

  // running segment sum across consecutive tiles of this wave: node id (wave uniform) + NQ output columns per lane
  // (the gated message row [H | 3 H | 5 H] is exactly an `out` row: column 64 q + lane)
  constexpr int NQ = (D + 63) / 64;
  // LDS row stride of the transposed tile (floats): rows stay 16-byte aligned, so a lane stores its 4 channels x (2l+1)
  // components of a degree -- contiguous in the output row -- as 2l+1 ds_write_b128 (18 per tile instead of 288 b32 stores
  // with 2-4 way bank conflicts); D + 4 = 73 16-byte units per row for H = 32: the 16 rows of a lane group fall on 16 different bank
  // quads.  The column reads of the run sums are consecutive lanes -> consecutive words for any stride.
  constexpr int RS = D + 4;
#if E3_MSG_STAMP
  uint32_t st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_t = (uint32_t)__builtin_readcyclecounter();
#define E3_STAMP(i) { const uint32_t t_ = (uint32_t)__builtin_readcyclecounter(); st_acc[i] += t_ - st_t; st_t = t_; }
#else
#define E3_STAMP(i)
#endif
  int cur = -1;
  float carry[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) carry[q] = 0.f;
  // (vmcnt is in-order: a wait for ANY vector-memory operation issued after a flush also waits for the acknowledgement of
  // its atomics, a round trip to the memory side.  The flush must therefore not reload anything from scratch -- the lane
  // id is regenerated (v_mbcnt) instead of kept, and the row address is scalar base + lane offset, so that the compiler
  // has no `out + lane` pointer pair to hoist out of the tile loop and spill.)
  auto flush = [&]() {
    if (cur >= 0) {
      int ln;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      float* o = out + (int64_t)cur * ldo;  // wave uniform
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (64 * q + ln < D) __builtin_amdgcn_global_atomic_fadd_f32(o + (64 * q + ln), carry[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) carry[q] = 0.f;
  };

  // The edge ids of a tile (16 src, 16 dst) are copied into LDS one tile ahead by a 4-byte LDS-DMA issued together with the
  // previous tile's gather copies (lanes 0-15: src, 16-31: dst): they land under the wait the
  // gather needs anyway and occupy no register across the products.  (As prefetched VGPRs they were spilled right after
  // the load -- `global_load; s_waitcnt vmcnt(0); scratch_store`, twice per tile -- and reloaded behind the atomics.)
  auto copy_ids = [&](int tile, int ln) {
    const int row0 = __builtin_amdgcn_readfirstlane(tile * 16);  // (pinned to SGPRs: as vector induction variables they
    const int nrows = __builtin_amdgcn_readfirstlane(Ei - row0 < 16 ? Ei - row0 : 16);  // get spilled and reloaded here)
    const int jl = ln & 15;
    const int e = row0 + (jl < nrows ? jl : nrows - 1);
    // two exec-masked copies with scalar bases (a per-lane choice between the two pointers becomes a 64-bit VGPR select
    // whose operands get hoisted and spilled)
    if (ln < 16) __builtin_amdgcn_global_load_lds((glb_void_t*)(src + e), (lds_void_t*)idbuf, 4, 0, 0);
    else if (ln < 32) __builtin_amdgcn_global_load_lds((glb_void_t*)(dst + e), (lds_void_t*)idbuf, 4, 0, 0);
  };
  // outer = this workgroup's chunks, inner = the tiles of this wave's block of the chunk.
  // (A workgroup barrier per tile, so that the waves share one weight stream through L1, measured 26.9 vs 26.5 ms.)
  const int chunk = 4 * blk;
  const int n_outer = (tiles_per_xcd + chunk * per_xcd - 1) / (chunk * per_xcd);
  for (int ob = 0; ob < n_outer; ++ob) {
    const int b0 = __builtin_amdgcn_readfirstlane(xcd_lo + (ob * per_xcd + wg_idx) * chunk + wave * blk);
    const int b1 = __builtin_amdgcn_readfirstlane(b0 + blk < xcd_hi ? b0 + blk : xcd_hi);
    if (b0 < b1) {  // the block's first tile: its ids are copied now
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      wave_sync_lds();
      copy_ids(b0, lane);
      wait_vm0();
      wave_sync_lds();
    }
    for (int tile = b0; tile < b1; ++tile) {
      const int row0 = __builtin_amdgcn_readfirstlane(tile * 16);
      const int nrows = __builtin_amdgcn_readfirstlane(Ei - row0 < 16 ? Ei - row0 : 16);
      int lt;  // lane id, regenerated per tile (the kernel-level copy is spilled across the products)
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lt));
      const int sid = idbuf[lt & 15], did = idbuf[16 + (lt & 15)];
      // per-tile opaque copies of loop-invariant addresses: without them LICM hoists ~50 table reads (200 registers) and
      // the block addresses out of the tile loop and spills them
      uint32_t woff = lt * 16;
      int tab0 = 0;
      asm volatile("" : "+v"(woff), "+v"(tab0));
      const float *n1p = n1tab + tab0, *n2p = n2tab + tab0, *wdp = wdtab + tab0;
      const int sd = (lt & 15) < nrows ? did : -1;

      // ---- stage the 16 h[src] rows by 16-byte LDS-DMA (the per-lane source address is the gather).  LDS image per wave:
      //      l_max 2: region A [row][1o | 2e] (2 H units of 16 bytes per row) then region B [row][0e] (H / 4 units);
      //      l_max 1: one region [row][0e | 1o] (H units).  Unit counts are powers of two, so a DMA instruction covers whole
      //      rows (row id by v_readlane: scalar address math) or 2^k rows (one shuffle), and no lane divides anything.
      // (the previous tile's LDS reads must have returned before the copies may land)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      wave_sync_lds();
      E3_STAMP(5)  // loop top: ids, reloads
      {
        int ls;  // lane id, regenerated: the kernel-level copy is spilled across the products
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ls));
        auto stage_region = [&](auto utag, auto otag, char* dstb) {
          constexpr int UNITS = decltype(utag)::value, SRCOFF = decltype(otag)::value;  // units per row, first source element
          if constexpr (UNITS >= 64) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rid = __builtin_amdgcn_readlane(sid, r);
              const char* rowp = h + ((int64_t)rid * ldh + SRCOFF) * ES;
#pragma unroll
              for (int k = 0; k < UNITS / 64; ++k)
                __builtin_amdgcn_global_load_lds((glb_void_t*)(rowp + (k * 64 + ls) * 16),
                                                 (lds_void_t*)(dstb + (r * UNITS + k * 64) * 16), 16, 0, 0);
            }
          } else {
            constexpr int RPI = 64 / UNITS;  // rows per instruction
            static_assert(RPI <= 16, "region rows shorter than 4 units are not supported");
            const int u = ls & (UNITS - 1), rl = ls / UNITS;
            int rid[16 / RPI];  // all shuffles first: they are LDS-pipe instructions, and hipcc guards every LDS access
#pragma unroll                  // behind an LDS-DMA in flight with vmcnt(0), which would serialise the copies
            for (int it = 0; it < 16 / RPI; ++it) rid[it] = __shfl(sid, it * RPI + rl);
#pragma unroll
            for (int it = 0; it < 16 / RPI; ++it)
              __builtin_amdgcn_global_load_lds((glb_void_t*)(h + ((int64_t)rid[it] * ldh + SRCOFF) * ES + u * 16),
                                               (lds_void_t*)(dstb + it * 1024), 16, 0, 0);
          }
        };
        // element counts per row: l_max 2: A = [1o | 2e] = 8 H, B = [0e] = H; l_max 1: 4 H
        char* wb = reinterpret_cast<char*>(wbuf);
        if (tile + 1 < b1) copy_ids(tile + 1, ls);
        if constexpr (LMAX == 2) {
          stage_region(std::integral_constant<int, 8 * H * ES / 16>{}, std::integral_constant<int, H>{}, wb);
          stage_region(std::integral_constant<int, H * ES / 16>{}, std::integral_constant<int, 0>{}, wb + 16 * 8 * H * ES);
        } else {
          stage_region(std::integral_constant<int, 4 * H * ES / 16>{}, std::integral_constant<int, 0>{}, wb);
        }
      }
      // ---- geometry while the copies fly ----
      float y[9], dist;
      {
        const float4 ps = pos4[sid], pd = pos4[did];
        if constexpr (PBC == kCell) {
          // The 18 cell entries are read from the kernel-argument segment HERE, once per tile: scalar loads into SGPRs that
          // are free again after the geometry (the offset passes through an empty asm, so the loads are not hoisted out
          // of the tile loop).  Held across the products they took the SGPRs that the tile loop's uniform values live
          // in, and those moved to VGPRs: the bf16 l_max = 1, H = 32 instantiation went from 104 to 131 VGPRs and lost
          // a wave per SIMD.
          typedef const __attribute__((address_space(4))) char* karg_ptr_t;
          const karg_ptr_t ka = (karg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
          int off = offsetof(MsgFusedKernarg, cell);
          asm volatile("" : "+s"(off));
          const __attribute__((address_space(4))) float* cp = (const __attribute__((address_space(4))) float*)(ka + off);
          PbcCell c;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            c.h[k] = cp[k];
            c.g[k] = cp[9 + k];
          }
          if constexpr (LMAX == 2) edge_sh<PBC>(ps, pd, y, dist, c); else edge_sh1<PBC>(ps, pd, y, dist, c);
        } else {
          if constexpr (LMAX == 2) edge_sh<PBC>(ps, pd, y, dist, box); else edge_sh1<PBC>(ps, pd, y, dist, box);
        }
      }
      f32x4 a0[T0], a1[TT][3], a2[LMAX == 2 ? TT : 1][5];
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < T0; ++t) a0[t] = zero4;
#pragma unroll
      for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) a1[t][c] = zero4;
#pragma unroll
      for (int t = 0; t < (LMAX == 2 ? TT : 1); ++t)
#pragma unroll
        for (int c = 0; c < 5; ++c) a2[t][c] = zero4;

      E3_STAMP(0)  // gather issue + geometry
      wait_vm0();
      wave_sync_lds();
      E3_STAMP(1)  // gather wait

      // ---- tensor product #1: x from the staged rows, dst half as accumulator initial values ----
      {
        // (every phase regenerates the lane id it needs: v_mbcnt costs two instructions, a lane-derived value kept across
        // the products costs a register there or a scratch reload here)
        int LL;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(LL));
        const int j = LL & 15, g = LL >> 4;
        TpCtx cx;
        cx.w = wrsrc;
        cx.wrole = 0;
        cx.woff = woff;
        cx.ud = U + (int64_t)did * G::UD + 4 * g;
        cx.wd = wdp + 4 * g;
        cx.dsc = dist * xs;
        auto xload = [&](auto l1tag, int ks, auto& x) {
          constexpr int L1 = decltype(l1tag)::value, D1 = 2 * L1 + 1;
          // first element of degree L1 in this lane's staged row (see the LDS image above), in elements
          const int e0 = LMAX == 2 ? (L1 == 0 ? 16 * 8 * H + j * H : j * 8 * H + (L1 == 1 ? 0 : 3 * H))
                                   : j * 4 * H + (L1 == 0 ? 0 : H);
          const char* xrow = reinterpret_cast<const char*>(wbuf) + e0 * ES;
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            if (16 * (2 * ks + p) < H) read_piece<D1, IO16>(xrow + (32 * ks + 16 * p + 4 * g) * D1 * ES, p, xs, x);
            else zero_piece<D1>(p, x);
          }
        };
        tp_core<LMAX, TT, true, IO16>(cx, y, xload, a0, a1, a2);
      }

      E3_STAMP(2)  // product #1
      // ---- gate #1; the messages stay in accumulator layout = the B-operand layout of product #2 ----
      // (norm1 already carries 1 / (sw1 xs)); row scale for the fp16 split: max |m| of the lane's edge -> 2^10
      float amax = 0.f;
      {
        int LL;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(LL));
        const int g = LL >> 4;
        const f32x4* nt = reinterpret_cast<const f32x4*>(n1p) + g;  // slot s at nt[4 s]
        auto gate_block = [&](auto dtag, auto& acc, const int slot, const int gslot) {
          constexpr int Dc = decltype(dtag)::value;
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            const f32x4 gn = nt[4 * (gslot + t)];
            float gt[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) gt[r] = sigmoid_(a0[gslot + t][r] * gn[r]);
#pragma unroll
            for (int c = 0; c < Dc; ++c) {
              const f32x4 nv = nt[4 * (slot + Dc * t + c)];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float v = acc[t][c][r] * nv[r] * gt[r];
                acc[t][c][r] = v;
                amax = fmaxf(amax, fabsf(v));
              }
            }
          }
        };
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const f32x4 nv = nt[4 * t];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sv = a0[t][r] * nv[r];
            const float v = sv * sigmoid_(sv);
            a0[t][r] = v;
            amax = fmaxf(amax, fabsf(v));
          }
        }
        gate_block(std::integral_constant<int, 3>{}, a1, G::slot0(1), TT);
        if constexpr (LMAX == 2) gate_block(std::integral_constant<int, 5>{}, a2, G::slot0(2), 2 * TT);
      }
      float srow = 1.0f, isrow = 1.0f;
      if constexpr (!IO16) {
        amax = fmaxf(amax, __shfl_xor(amax, 16));
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        srow = pow2_scale_from_bits(__builtin_bit_cast(uint32_t, amax), 10);
        isrow = 1.0f / srow;
      }

      // ---- park the (scaled) messages: slot q of lane l at wbuf[(q * 64 + l) * 4] ----
      wave_sync_lds();
      {
        int LL;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(LL));
        f32x4* pk = reinterpret_cast<f32x4*>(wbuf) + LL;
        auto sc4 = [&](const f32x4 v) {
          if constexpr (IO16) {  // bf16 storage: the messages between the two products are bf16 values
            f32x4 o;
            for (int r = 0; r < 4; ++r) o[r] = (float)(__bf16)v[r];
            return o;
          } else {
            return f32x4{v[0] * srow, v[1] * srow, v[2] * srow, v[3] * srow};
          }
        };
#pragma unroll
        for (int t = 0; t < TT; ++t) pk[64 * t] = sc4(a0[t]);
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
          for (int c = 0; c < 3; ++c) pk[64 * (TT + 3 * t + c)] = sc4(a1[t][c]);
        if constexpr (LMAX == 2) {
#pragma unroll
          for (int t = 0; t < TT; ++t)
#pragma unroll
            for (int c = 0; c < 5; ++c) pk[64 * (4 * TT + 5 * t + c)] = sc4(a2[t][c]);
        }
      }
      wave_sync_lds();

      E3_STAMP(3)  // gate #1 + park
      // ---- tensor product #2 ----
#pragma unroll
      for (int t = 0; t < T0; ++t) a0[t] = zero4;
#pragma unroll
      for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) a1[t][c] = zero4;
#pragma unroll
      for (int t = 0; t < (LMAX == 2 ? TT : 1); ++t)
#pragma unroll
        for (int c = 0; c < 5; ++c) a2[t][c] = zero4;
      {
        TpCtx cx;
        cx.w = wrsrc; cx.wrole = G::nblk() * 2048; cx.woff = woff; cx.ud = nullptr; cx.wd = nullptr; cx.dsc = 0.f;
        int LL;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(LL));
        const f32x4* pk = reinterpret_cast<const f32x4*>(wbuf) + LL;
        auto xload = [&](auto l1tag, int ks, auto& x) {
          constexpr int L1 = decltype(l1tag)::value, D1 = 2 * L1 + 1;
          constexpr int S0 = L1 == 0 ? 0 : L1 == 1 ? TT : 4 * TT;  // first parked slot of degree L1
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int t = 2 * ks + p;
#pragma unroll
            for (int a = 0; a < D1; ++a) {
              f32x4 v = zero4;
              if (t < TT) v = pk[64 * (S0 + D1 * t + a)];
#pragma unroll
              for (int r = 0; r < 4; ++r) x[4 * p + r][a] = v[r];
            }
          }
        };
        tp_core<LMAX, TT, false, IO16>(cx, y, xload, a0, a1, a2);
      }

      E3_STAMP(4)  // product #2
      // ---- gate #2, then the segment sum: the whole gated tile goes to LDS as [row][output column] (the accumulators are
      //      dead from here on), lane = output column walks the 16 rows and adds runs of equal dst; the last run is carried
      //      into the wave's next tile ----
      {
        int LL;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(LL));
        const int j = LL & 15, g = LL >> 4;
        const f32x4* nt2 = reinterpret_cast<const f32x4*>(n2p) + g;
        wave_sync_lds();
        float* wp = wbuf + j * RS + 4 * g;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const f32x4 nv = nt2[4 * t];
          f32x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sv = a0[t][r] * nv[r] * isrow;
            o[r] = sv * sigmoid_(sv);
          }
          *reinterpret_cast<f32x4*>(wp + 16 * t) = o;
        }
        auto put_block = [&](auto dtag, auto& acc, const int slot, const int gslot, float* wq) {
          constexpr int Dc = decltype(dtag)::value;
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            const f32x4 gn = nt2[4 * (gslot + t)];
            float gt[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) gt[r] = sigmoid_(a0[gslot + t][r] * gn[r] * isrow) * isrow;
            float o[4 * Dc];  // the lane's 4 channels x Dc components: one contiguous piece of the output row
#pragma unroll
            for (int c = 0; c < Dc; ++c) {
              const f32x4 nv = nt2[4 * (slot + Dc * t + c)];
#pragma unroll
              for (int r = 0; r < 4; ++r) o[r * Dc + c] = acc[t][c][r] * nv[r] * gt[r];
            }
            f32x4* dq = reinterpret_cast<f32x4*>(wq + 16 * t * Dc);
#pragma unroll
            for (int k = 0; k < Dc; ++k) dq[k] = f32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
          }
        };
        put_block(std::integral_constant<int, 3>{}, a1, G::slot0(1), TT, wbuf + j * RS + H + 12 * g);
        if constexpr (LMAX == 2) put_block(std::integral_constant<int, 5>{}, a2, G::slot0(2), 2 * TT, wbuf + j * RS + 4 * H + 20 * g);
        wave_sync_lds();
        E3_STAMP(6)  // gate #2 + transposed writes
        // from here to the next tile's gather nothing may wait on vmcnt behind a flush (see `flush`): the lane id is
        // regenerated, the next tile's ids are made to have arrived
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const float* sp = wbuf + ln;
#pragma unroll
        for (int rb = 0; rb < 16; rb += 4) {
          float v[4][NQ];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[rr][q] = (64 * q + ln < D) ? sp[(rb + rr) * RS + 64 * q] : 0.f;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int dn = __builtin_amdgcn_readlane(sd, rb + rr);
            if (dn >= 0) {
              if (dn != cur) {
                flush();
                cur = dn;
              }
#pragma unroll
              for (int q = 0; q < NQ; ++q) carry[q] += v[rr][q];
            }
          }
        }
      }
      E3_STAMP(7)  // run sums + flushes
    }
    flush();  // the wave's next tile is not the successor of this one
    cur = -1;
  }
#if E3_MSG_STAMP
  if (lane == 0)
    for (int i = 0; i < 8; ++i) atomicAdd(&g_msg_stamps[i], (unsigned long long)st_acc[i]);
#endif
#undef E3_STAMP
}

// MsgFusedKernarg against the kernel's signature (see the struct)
static_assert(std::is_same_v<decltype(&msg_fused_kernel<1, 1, false, kCell>),
                             void (*)(decltype(MsgFusedKernarg::hv), decltype(MsgFusedKernarg::ldh), decltype(MsgFusedKernarg::pos4),
                                      decltype(MsgFusedKernarg::src), decltype(MsgFusedKernarg::dst), decltype(MsgFusedKernarg::E),
                                      decltype(MsgFusedKernarg::packed), decltype(MsgFusedKernarg::U),
                                      decltype(MsgFusedKernarg::in_scale), decltype(MsgFusedKernarg::out),
                                      decltype(MsgFusedKernarg::ldo), decltype(MsgFusedKernarg::blk),
                                      decltype(MsgFusedKernarg::cell))>,
              "MsgFusedKernarg must list the parameters of msg_fused_kernel in order");
static_assert(offsetof(MsgFusedKernarg, cell) == 92 && sizeof(PbcCell) == 72, "the cell follows `int blk` at byte 92");

// The instantiations of one storage type, their addresses taken where they are instantiated (bf16 storage for H >= 32 only:
// the [0e] region of a staged row must be at least 4 units of 16 bytes)
template <bool IO16, int PBC>
static void msg_fused_row(const void* (&row)[kMsgShapes]) {
#define E3_MSG_FUSED_PTR(I, LMAX, TT) \
  if constexpr (IO16 && TT < 2) row[I] = nullptr; else row[I] = (const void*)msg_fused_kernel<LMAX, TT, IO16, PBC>;
  E3_MSG_SHAPES(E3_MSG_FUSED_PTR)
#undef E3_MSG_FUSED_PTR
}
template <bool IO16>
static MsgFusedKernels msg_fused_kernels() {
  MsgFusedKernels t;
  msg_fused_row<IO16, kOpen>(t.k[kOpen]);
  msg_fused_row<IO16, kBox>(t.k[kBox]);
  msg_fused_row<IO16, kCell>(t.k[kCell]);
  return t;
}
