// Morton-range halo (sharding.MortonPartition / MortonHalo): rank q owns the cells whose Morton key lies in
// [s_q, s_{q+1}); an owned particle goes to every other rank that owns a cell of [cell(p - r), cell(p + r)]^3.
// Spec: include/e3gnn.h, e3_morton_select_count.  Integer / HBM work, no MFMA: one thread per particle builds a 64-bit mask
// of destination ranks in registers (owner of a cell = branch-free binary search of its key in the splitters, staged once
// per block in LDS); a particle whose range is one cell costs one search, the others 8 to 27 (cells are between r and 2r wide
// unless the grid is capped, so 2 or 3 per axis is the rule).  Counting and placement are e3_select.h's, as in e3_halo.hip:
// one 64-bit ballot + popcount per destination and wave -- only for the destinations some lane of the wave has --, the waves
// of a block summed in LDS into a rank-major [n_ranks, n_blocks] array, one exclusive scan, and a fill pass that recomputes
// the predicate: the output is grouped by destination with ascending particle ids inside a group, the order of
// mask.nonzero() on a rank-major [n_ranks, n] mask.
#include "e3_select.h"

#include <cmath>

namespace e3 {

// by value as a kernel argument.  split[k] = s_{k+1} for k < n_ranks - 1, 0xFFFFFFFF beyond (no key reaches it): the owner
// of a key is the number of entries <= key
struct MortonDev {
  float lo[3], inv[3];
  int n[3];
  float r;
  int n_ranks, self;
  uint32_t split[E3_MORTON_MAX_RANKS];
};

__device__ __forceinline__ float3 load3(const float* __restrict__ pos, const int64_t i) {
  return make_float3(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2]);
}

// thread 0 copies the splitters with constant indices (wave-uniform reads of the argument block, no per-lane indexing)
__device__ __forceinline__ void stage_splitters(const MortonDev& m, uint32_t* __restrict__ s_split) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < E3_MORTON_MAX_RANKS; ++k) s_split[k] = m.split[k];
  }
}

// number of staged splitters <= key: 6 steps over the 63 live slots of the padded array
__device__ __forceinline__ int owner_of_key(const uint32_t* __restrict__ s_split, const uint32_t key) {
  int q = 0;
#pragma unroll
  for (int step = E3_MORTON_MAX_RANKS / 2; step > 0; step >>= 1) q += s_split[q + step - 1] <= key ? step : 0;
  return q;
}

// destination ranks of one owned particle (bit q), this rank's own bit cleared
__device__ __forceinline__ unsigned long long dest_mask(const float3 p, const MortonDev& m,
                                                        const uint32_t* __restrict__ s_split) {
  const int x0 = cell_of(__fsub_rn(p.x, m.r), m.lo[0], m.inv[0], m.n[0]), x1 = cell_of(__fadd_rn(p.x, m.r), m.lo[0], m.inv[0], m.n[0]);
  const int y0 = cell_of(__fsub_rn(p.y, m.r), m.lo[1], m.inv[1], m.n[1]), y1 = cell_of(__fadd_rn(p.y, m.r), m.lo[1], m.inv[1], m.n[1]);
  const int z0 = cell_of(__fsub_rn(p.z, m.r), m.lo[2], m.inv[2], m.n[2]), z1 = cell_of(__fadd_rn(p.z, m.r), m.lo[2], m.inv[2], m.n[2]);
  unsigned long long mask = 0;
  if (x0 == x1 && y0 == y1 && z0 == z1) {   // one cell (cells wider than 2 r): one search
    mask = 1ull << owner_of_key(s_split, morton3(x0, y0, z0));
  } else {
    for (int z = z0; z <= z1; ++z) {
      const uint32_t kz = spread3((uint32_t)z) << 2;
      for (int y = y0; y <= y1; ++y) {
        const uint32_t kyz = kz | (spread3((uint32_t)y) << 1);
        for (int x = x0; x <= x1; ++x) mask |= 1ull << owner_of_key(s_split, kyz | spread3((uint32_t)x));
      }
    }
  }
  return mask & ~(1ull << m.self);
}

// OR over the wave, wave-uniform; every lane of the wave must call it
__device__ __forceinline__ unsigned long long wave_or(const unsigned long long v) {
  if (__ballot(v != 0) == 0) return 0;
  uint32_t a = (uint32_t)v, b = (uint32_t)(v >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a |= __shfl_xor(a, o);
    b |= __shfl_xor(b, o);
  }
  a = __builtin_amdgcn_readfirstlane(a);
  b = __builtin_amdgcn_readfirstlane(b);
  return ((unsigned long long)b << 32) | a;
}

__global__ __launch_bounds__(kSelectThreads) void morton_keys_kernel(const float* __restrict__ pos, int64_t n, const MortonDev m,
                                                                     int32_t* __restrict__ keys) {
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  if (i >= n) return;
  const float3 p = load3(pos, i);
  keys[i] = (int32_t)morton3(cell_of(p.x, m.lo[0], m.inv[0], m.n[0]), cell_of(p.y, m.lo[1], m.inv[1], m.n[1]),
                             cell_of(p.z, m.lo[2], m.inv[2], m.n[2]));
}

// the mask of this thread's particle and, in wcnt[wave][q], the number of lanes of each wave that send to q
__device__ __forceinline__ unsigned long long block_masks(const float* __restrict__ pos, const int64_t n, const MortonDev& m,
                                                          uint32_t* __restrict__ s_split,
                                                          int32_t (*__restrict__ wcnt)[E3_MORTON_MAX_RANKS]) {
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  stage_splitters(m, s_split);
  wcnt[wave][lane] = 0;
  __syncthreads();
  const unsigned long long mask = i < n ? dest_mask(load3(pos, i), m, s_split) : 0ull;
  for (unsigned long long left = wave_or(mask); left; left &= left - 1) {
    const int q = __builtin_ctzll(left);
    const unsigned long long b = __ballot((mask >> q) & 1);
    if (lane == 0) wcnt[wave][q] = __popcll(b);
  }
  __syncthreads();
  return mask;
}

// per (rank, block) hit counts, rank-major: bcnt[q * nb + b]
__global__ __launch_bounds__(kSelectThreads) void morton_count_kernel(const float* __restrict__ pos, int64_t n, const MortonDev m,
                                                                      int32_t* __restrict__ bcnt) {
  __shared__ uint32_t s_split[E3_MORTON_MAX_RANKS];
  __shared__ int32_t wcnt[kSelectWaves][E3_MORTON_MAX_RANKS];
  block_masks(pos, n, m, s_split, wcnt);
  store_block_counts(wcnt, m.n_ranks, bcnt);
}

__global__ __launch_bounds__(kSelectThreads) void morton_fill_kernel(const float* __restrict__ pos, int64_t n, const MortonDev m,
                                                                     const int32_t* __restrict__ off, int64_t total,
                                                                     int32_t* __restrict__ idx) {
  __shared__ uint32_t s_split[E3_MORTON_MAX_RANKS];
  __shared__ int32_t wcnt[kSelectWaves][E3_MORTON_MAX_RANKS];
  const unsigned long long mask = block_masks(pos, n, m, s_split, wcnt);
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes < this one
  for (unsigned long long left = wave_or(mask); left; left &= left - 1) {
    const int q = __builtin_ctzll(left);
    const bool in = (mask >> q) & 1;
    const unsigned long long b = __ballot(in);
    if (!in) continue;
    const int64_t o = select_slot(off, wcnt, q, wave, b, below);
    if (o >= total) continue;   // only a caller that changed the inputs between the two calls gets here
    idx[o] = (int32_t)i;
  }
}

static bool morton_sizes_ok(int64_t n, int n_ranks) { return select_sizes_ok(n, n_ranks, 1, E3_MORTON_MAX_RANKS); }

// host: the validated grid (finite non-empty box, n_cells powers of two in [1, 128])
static int morton_grid(const float lo[3], const float hi[3], const int32_t n_cells[3], MortonDev* m) {
  if (!lo || !hi || !n_cells) return E3_ERR_INVALID_ARG;
  *m = MortonDev{};
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(lo[a] < hi[a])) return E3_ERR_INVALID_ARG;
    const float L = hi[a] - lo[a];
    const int n = n_cells[a];
    if (!std::isfinite(L) || n < 1 || n > 128 || (n & (n - 1))) return E3_ERR_INVALID_ARG;
    m->lo[a] = lo[a];
    m->inv[a] = (float)n / L;
    m->n[a] = n;
  }
  return E3_OK;
}

// host: grid + selection parameters (cells at least r wide on an axis that has several, splitters non-decreasing from 0)
static int morton_dev(const float lo[3], const float hi[3], const int32_t n_cells[3], float r, const int32_t* splitters,
                      int n_ranks, int self_rank, MortonDev* m) {
  const int st = morton_grid(lo, hi, n_cells, m);
  if (st != E3_OK) return st;
  if (n_ranks < 1 || n_ranks > E3_MORTON_MAX_RANKS || self_rank < 0 || self_rank >= n_ranks || !splitters) return E3_ERR_INVALID_ARG;
  if (!std::isfinite(r) || !(r > 0.0f)) return E3_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a)
    if (n_cells[a] > 1 && (hi[a] - lo[a]) / (float)n_cells[a] < r) return E3_ERR_INVALID_ARG;   // exact: n is a power of two
  if (splitters[0] != 0) return E3_ERR_INVALID_ARG;
  for (int q = 0; q < n_ranks; ++q)
    if (splitters[q + 1] < splitters[q]) return E3_ERR_INVALID_ARG;
  m->r = r;
  m->n_ranks = n_ranks;
  m->self = self_rank;
  for (int k = 0; k < E3_MORTON_MAX_RANKS; ++k) m->split[k] = k < n_ranks - 1 ? (uint32_t)splitters[k + 1] : 0xFFFFFFFFu;
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_morton_keys(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], int32_t* keys,
                   void* stream) {
  MortonDev m;
  const int st = morton_grid(lo, hi, n_cells, &m);
  if (st != E3_OK) return st;
  if (n < 0 || n >= 0x7fffffffLL || (n > 0 && (!pos || !keys))) return E3_ERR_INVALID_ARG;
  if (n == 0) return E3_OK;
  hipLaunchKernelGGL(morton_keys_kernel, dim3(select_blocks(n)), dim3(kSelectThreads), 0, (hipStream_t)stream, pos, n, m,
                     keys);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int64_t e3_morton_select_workspace_bytes(int64_t n, int n_ranks) {
  if (!morton_sizes_ok(n, n_ranks)) return -1;
  return (int64_t)select_ws(n, n_ranks).total;
}

int e3_morton_select_count(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], float r,
                           const int32_t* splitters, int n_ranks, int self_rank, int32_t* counts, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  if (!morton_sizes_ok(n, n_ranks)) return E3_ERR_INVALID_ARG;
  MortonDev m;
  const int st = morton_dev(lo, hi, n_cells, r, splitters, n_ranks, self_rank, &m);
  if (st != E3_OK) return st;
  if ((n > 0 && !pos) || !counts || !workspace) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_ranks);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    E3_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_ranks * 4, s));
    return E3_OK;
  }
  const int nb = select_blocks(n);
  return select_count(workspace, w, nb, n_ranks, counts, s, [&](int32_t* bcnt) {
    hipLaunchKernelGGL(morton_count_kernel, dim3(nb), dim3(kSelectThreads), 0, s, pos, n, m, bcnt);
  });
}

int e3_morton_select_fill(const float* pos, int64_t n, const float lo[3], const float hi[3], const int32_t n_cells[3], float r,
                          const int32_t* splitters, int n_ranks, int self_rank, int64_t total, int32_t* idx, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  if (!morton_sizes_ok(n, n_ranks)) return E3_ERR_INVALID_ARG;
  MortonDev m;
  const int st = morton_dev(lo, hi, n_cells, r, splitters, n_ranks, self_rank, &m);
  if (st != E3_OK) return st;
  if (total < 0) return E3_ERR_INVALID_ARG;
  if (n == 0 || total == 0) return E3_OK;
  if (!pos || !idx || !workspace) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_ranks);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(morton_fill_kernel, dim3(select_blocks(n)), dim3(kSelectThreads), 0, (hipStream_t)stream, pos, n, m,
                     (const int32_t*)(static_cast<char*>(workspace) + w.off), total, idx);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
