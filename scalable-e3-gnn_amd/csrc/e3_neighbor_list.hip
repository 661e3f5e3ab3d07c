// Verlet neighbour list (neighbor_list.NeighborList): a graph built once at r + skin is cut down to the pairs within r at the
// current positions, and the largest displacement since the build is reduced on the way -- include/e3gnn.h, e3_nl_update.
// Integer / HBM work: no MFMA.  Three launches and one scan: gather + displacement (a thread per node), count (needs every
// gathered position), exclusive sum, fill.  Count and fill walk the stored edges with a 16-lane group per row, four rows per
// wave: the index reads along a row are coalesced and the fill compacts with the group's bits of a wave-wide ballot, which
// keeps the order of the row.  e3_nl_update_split is the same walk for the local cloud of a shard: it also drops the ghost
// rows and splits the kept edges by the ownership of their src (two ballots, two scans).
#include "e3_common.h"

namespace e3 {

constexpr int kNlThreads = 256;
constexpr int kNlGroup = 16;                        // lanes per row
constexpr int kNlRows = kNlThreads / kNlGroup;      // rows per block

// the edge test of the builder (e3_rg_sort_count) on the edge vector of the geometry kernels
template <int MODE>
__device__ __forceinline__ bool nl_keep(const float4 pj, const float4 pi, const typename PbcArg<MODE>::type& box,
                                        const float r2) {
  float dx, dy, dz;
  edge_rel<MODE>(pj, pi, box, dx, dy, dz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) <= r2;
}

// pos4_out[i] = (pos[perm[i]], 0); stats[0] = max_i of the uint bits (sign cleared) of |minimum image of pos4_out[i] - ref[i]|^2
template <int MODE>
__global__ void __launch_bounds__(kNlThreads)
nl_gather_kernel(const float* __restrict__ pos, const int32_t* __restrict__ perm, const float4* __restrict__ ref,
                 const int64_t N, const typename PbcArg<MODE>::type box, float4* __restrict__ pos4_out,
                 uint32_t* __restrict__ stats) {
  __shared__ uint32_t wave_max[kNlThreads / 64];
  const int64_t i = blockIdx.x * (int64_t)kNlThreads + threadIdx.x;
  uint32_t m = 0;
  if (i < N) {
    const int64_t p = perm[i];
    const float4 x = make_float4(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], 0.f);
    pos4_out[i] = x;
    float dx, dy, dz;
    edge_rel<MODE>(x, ref[i], box, dx, dy, dz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    m = __float_as_uint(d2) & 0x7fffffffu;   // non-negative floats order as their bits; a NaN orders above +inf
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNlThreads / 64; ++w) m = max(m, wave_max[w]);
    if (m) atomicMax(&stats[0], m);
  }
}

// FILL = false: cnt[i] = kept edges of row i (cnt[N] = 0: the exclusive scan leaves the total there).
// FILL = true : the kept edges of row i to src_out / dst_out from out_ptr[i] on, in the row's order; stats[1] = out_ptr[N].
template <int MODE, bool FILL>
__global__ void __launch_bounds__(kNlThreads)
nl_prune_kernel(const float4* __restrict__ pos4, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                const int64_t N, const float r2, const typename PbcArg<MODE>::type box, int32_t* __restrict__ cnt,
                const int32_t* __restrict__ out_ptr, int32_t* __restrict__ src_out, int32_t* __restrict__ dst_out,
                uint32_t* __restrict__ stats) {
  const int sub = threadIdx.x & (kNlGroup - 1);
  const int shift = threadIdx.x & 63 & ~(kNlGroup - 1);   // first lane of this group inside its wave
  const int64_t i = blockIdx.x * (int64_t)kNlRows + threadIdx.x / kNlGroup;
  if (FILL && i == 0 && sub == 0) stats[1] = (uint32_t)out_ptr[N];
  int b = 0, e = 0;
  float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < N) { b = rowptr[i]; e = rowptr[i + 1]; pi = pos4[i]; }
  // the trip count is the longest row of the wave, so every lane is at the ballot
  int len = e - b;
  len = max(len, __shfl_xor(len, 16));
  len = max(len, __shfl_xor(len, 32));
  int kept = FILL && i < N ? out_ptr[i] : 0;
  for (int base = 0; base < len; base += kNlGroup) {
    const int p = b + base + sub;
    bool ok = false;
    int s = 0;
    if (p < e) {
      s = src[p];
      ok = nl_keep<MODE>(pos4[s], pi, box, r2);
    }
    const unsigned mask = (unsigned)(__ballot(ok) >> shift) & ((1u << kNlGroup) - 1u);
    if (FILL && ok) {
      const int o = kept + __popc(mask & ((1u << sub) - 1u));
      src_out[o] = s;
      dst_out[o] = (int32_t)i;
    }
    kept += __popc(mask);
  }
  if (!FILL && sub == 0 && i <= N) cnt[i] = kept;
}

static size_t nl_align(size_t b) { return (b + 255) / 256 * 256; }

template <int MODE>
static int nl_update(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                     int64_t N, int64_t E, float r, const typename PbcArg<MODE>::type& box, float* pos4_out,
                     int32_t* rowptr_out, int32_t* src_out, int32_t* dst_out, uint32_t* stats, void* workspace,
                     hipStream_t s) {
  if (N < 0 || E < 0 || N + 1 > 0x7fffffffLL || E > 0x7fffffffLL || !(r > 0.0f) || !(r < 3.0e38f))
    return E3_ERR_INVALID_ARG;
  if (!rowptr_out || !stats || !workspace) return E3_ERR_INVALID_ARG;
  if (N > 0 && (!pos || !perm || !ref_pos4 || !rowptr || !pos4_out)) return E3_ERR_INVALID_ARG;
  if (E > 0 && (!src || !src_out || !dst_out)) return E3_ERR_INVALID_ARG;
  E3_HIP_CHECK(hipMemsetAsync(stats, 0, 2 * sizeof(uint32_t), s));
  if (N == 0) {
    E3_HIP_CHECK(hipMemsetAsync(rowptr_out, 0, sizeof(int32_t), s));
    return E3_OK;
  }
  const float r2 = r * r;  // fp32 product, as the builder's
  char* w = static_cast<char*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(w);
  void* temp = w + nl_align((size_t)(N + 1) * 4);
  const float4* p4 = reinterpret_cast<const float4*>(pos4_out);
  const unsigned node_blocks = (unsigned)((N + kNlThreads - 1) / kNlThreads);
  const unsigned row_blocks = (unsigned)((N + 1 + kNlRows - 1) / kNlRows);
  hipLaunchKernelGGL((nl_gather_kernel<MODE>), dim3(node_blocks), dim3(kNlThreads), 0, s, pos, perm,
                     reinterpret_cast<const float4*>(ref_pos4), N, box, reinterpret_cast<float4*>(pos4_out), stats);
  hipLaunchKernelGGL((nl_prune_kernel<MODE, false>), dim3(row_blocks), dim3(kNlThreads), 0, s, p4, rowptr, src, N, r2, box,
                     cnt, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, stats);
  E3_HIP_CHECK(exclusive_sum(temp, scan_temp_bytes(N + 1), cnt, rowptr_out, N + 1, s));
  hipLaunchKernelGGL((nl_prune_kernel<MODE, true>), dim3(row_blocks), dim3(kNlThreads), 0, s, p4, rowptr, src, N, r2, box,
                     (int32_t*)nullptr, rowptr_out, src_out, dst_out, stats);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// The prune of an open local cloud [owned | ghosts] and the split of sharding.Halo.split_graph in one walk over the stored
// edges (e3_nl_update_split): a ghost row keeps nothing, an owned row keeps what nl_keep keeps, and every kept edge also
// goes to the interior (owned src) or the boundary (ghost src) list.  The group's bits of two ballots -- kept, kept with a
// ghost src -- give both per-row counts and, in the fill pass, the three write positions as popcounts of the lower bits.
// FILL = false: cnt_k[i] / cnt_b[i] = kept / boundary edges of row i (element N = 0: the scans leave the totals there).
// FILL = true : the lists from out_k[i] / out_b[i] / out_k[i] - out_b[i] on, in the row's order; stats[1..3] = the totals.
template <bool FILL>
__global__ void __launch_bounds__(kNlThreads)
nl_split_kernel(const float4* __restrict__ pos4, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                const uint8_t* __restrict__ ghost, const int64_t N, const float r2, int32_t* __restrict__ cnt_k,
                int32_t* __restrict__ cnt_b, const int32_t* __restrict__ out_k, const int32_t* __restrict__ out_b,
                int32_t* __restrict__ src_k, int32_t* __restrict__ dst_k, int32_t* __restrict__ src_i,
                int32_t* __restrict__ dst_i, int32_t* __restrict__ src_b, int32_t* __restrict__ dst_b,
                uint32_t* __restrict__ stats) {
  const int sub = threadIdx.x & (kNlGroup - 1);
  const int shift = threadIdx.x & 63 & ~(kNlGroup - 1);   // first lane of this group inside its wave
  const int64_t i = blockIdx.x * (int64_t)kNlRows + threadIdx.x / kNlGroup;
  if (FILL && i == 0 && sub == 0) {
    const int32_t k = out_k[N], nb = out_b[N];
    stats[1] = (uint32_t)k; stats[2] = (uint32_t)(k - nb); stats[3] = (uint32_t)nb;
  }
  int b = 0, e = 0;
  float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < N && !ghost[i]) { b = rowptr[i]; e = rowptr[i + 1]; pi = pos4[i]; }   // a ghost row is an empty row
  // the trip count is the longest row of the wave, so every lane is at the ballots
  int len = e - b;
  len = max(len, __shfl_xor(len, 16));
  len = max(len, __shfl_xor(len, 32));
  int kept = FILL && i < N ? out_k[i] : 0;
  int bnd = FILL && i < N ? out_b[i] : 0;
  for (int base = 0; base < len; base += kNlGroup) {
    const int p = b + base + sub;
    bool ok = false, gs = false;
    int s = 0;
    if (p < e) {
      s = src[p];
      ok = nl_keep<kOpen>(pos4[s], pi, PbcBox{}, r2);
      gs = ok && ghost[s];
    }
    const unsigned mk = (unsigned)(__ballot(ok) >> shift) & ((1u << kNlGroup) - 1u);
    const unsigned mb = (unsigned)(__ballot(gs) >> shift) & ((1u << kNlGroup) - 1u);
    if (FILL && ok) {
      const unsigned below = (1u << sub) - 1u;
      const int qk = kept + __popc(mk & below);
      const int qb = bnd + __popc(mb & below);
      src_k[qk] = s;
      dst_k[qk] = (int32_t)i;
      if (gs) { src_b[qb] = s; dst_b[qb] = (int32_t)i; }
      else { src_i[qk - qb] = s; dst_i[qk - qb] = (int32_t)i; }
    }
    kept += __popc(mk);
    bnd += __popc(mb);
  }
  if (!FILL && sub == 0 && i <= N) { cnt_k[i] = kept; cnt_b[i] = bnd; }
}

}  // namespace e3

using namespace e3;

extern "C" {

int64_t e3_nl_update_split_workspace_bytes(int64_t N) {
  if (N < 0 || N + 1 > 0x7fffffffLL) return -1;
  return (int64_t)(3 * nl_align((size_t)(N + 1) * 4) + nl_align(scan_temp_bytes(N + 1)));
}

int e3_nl_update_split(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                       const uint8_t* is_ghost, int64_t N, int64_t E, float r, float* pos4_out, int32_t* rowptr_out,
                       int32_t* src_out, int32_t* dst_out, int32_t* src_interior, int32_t* dst_interior,
                       int32_t* src_boundary, int32_t* dst_boundary, uint32_t* stats, void* workspace, void* stream) {
  if (N < 0 || E < 0 || N + 1 > 0x7fffffffLL || E > 0x7fffffffLL || !(r > 0.0f) || !(r < 3.0e38f))
    return E3_ERR_INVALID_ARG;
  if (!rowptr_out || !stats || !workspace) return E3_ERR_INVALID_ARG;
  if (N > 0 && (!pos || !perm || !ref_pos4 || !rowptr || !pos4_out || !is_ghost)) return E3_ERR_INVALID_ARG;
  if (E > 0 && (!src || !src_out || !dst_out || !src_interior || !dst_interior || !src_boundary || !dst_boundary))
    return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  E3_HIP_CHECK(hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), s));
  if (N == 0) {
    E3_HIP_CHECK(hipMemsetAsync(rowptr_out, 0, sizeof(int32_t), s));
    return E3_OK;
  }
  const float r2 = r * r;  // fp32 product, as the builder's
  const size_t arr = nl_align((size_t)(N + 1) * 4);
  char* w = static_cast<char*>(workspace);
  int32_t *ck = reinterpret_cast<int32_t*>(w), *cb = reinterpret_cast<int32_t*>(w + arr),
          *ob = reinterpret_cast<int32_t*>(w + 2 * arr);
  void* temp = w + 3 * arr;
  const float4* p4 = reinterpret_cast<const float4*>(pos4_out);
  const unsigned node_blocks = (unsigned)((N + kNlThreads - 1) / kNlThreads);
  const unsigned row_blocks = (unsigned)((N + 1 + kNlRows - 1) / kNlRows);
  hipLaunchKernelGGL((nl_gather_kernel<kOpen>), dim3(node_blocks), dim3(kNlThreads), 0, s, pos, perm,
                     reinterpret_cast<const float4*>(ref_pos4), N, PbcBox{}, reinterpret_cast<float4*>(pos4_out), stats);
  hipLaunchKernelGGL((nl_split_kernel<false>), dim3(row_blocks), dim3(kNlThreads), 0, s, p4, rowptr, src, is_ghost, N, r2,
                     ck, cb, (const int32_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, stats);
  E3_HIP_CHECK(exclusive_sum(temp, scan_temp_bytes(N + 1), ck, rowptr_out, N + 1, s));
  E3_HIP_CHECK(exclusive_sum(temp, scan_temp_bytes(N + 1), cb, ob, N + 1, s));
  hipLaunchKernelGGL((nl_split_kernel<true>), dim3(row_blocks), dim3(kNlThreads), 0, s, p4, rowptr, src, is_ghost, N, r2,
                     (int32_t*)nullptr, (int32_t*)nullptr, rowptr_out, ob, src_out, dst_out, src_interior, dst_interior,
                     src_boundary, dst_boundary, stats);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int64_t e3_nl_workspace_bytes(int64_t N) {
  if (N < 0 || N + 1 > 0x7fffffffLL) return -1;
  return (int64_t)(nl_align((size_t)(N + 1) * 4) + nl_align(scan_temp_bytes(N + 1)));
}

int e3_nl_update(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                 int64_t N, int64_t E, float r, float* pos4_out, int32_t* rowptr_out, int32_t* src_out, int32_t* dst_out,
                 uint32_t* stats, void* workspace, void* stream) {
  return nl_update<kOpen>(pos, perm, ref_pos4, rowptr, src, N, E, r, PbcBox{}, pos4_out, rowptr_out, src_out, dst_out, stats,
                          workspace, (hipStream_t)stream);
}

int e3_nl_update_pbc(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                     int64_t N, int64_t E, float r, const float box[3], float* pos4_out, int32_t* rowptr_out,
                     int32_t* src_out, int32_t* dst_out, uint32_t* stats, void* workspace, void* stream) {
  if (!box_valid(box, 0.0f)) return E3_ERR_INVALID_ARG;
  return nl_update<kBox>(pos, perm, ref_pos4, rowptr, src, N, E, r, make_box(box), pos4_out, rowptr_out, src_out, dst_out,
                         stats, workspace, (hipStream_t)stream);
}

int e3_nl_update_cell(const float* pos, const int32_t* perm, const float* ref_pos4, const int32_t* rowptr, const int32_t* src,
                      int64_t N, int64_t E, float r, const float cell[9], float* pos4_out, int32_t* rowptr_out,
                      int32_t* src_out, int32_t* dst_out, uint32_t* stats, void* workspace, void* stream) {
  PbcCell c;
  if (!make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  return nl_update<kCell>(pos, perm, ref_pos4, rowptr, src, N, E, r, c, pos4_out, rowptr_out, src_out, dst_out, stats,
                          workspace, (hipStream_t)stream);
}

}  // extern "C"
