// Two-pass grouped selection, the scaffold shared by e3_halo.hip (group = halo entry) and e3_morton_halo.hip (group =
// destination rank).  One thread per particle; a count kernel leaves in wcnt[wave][g] how many lanes of each wave hit group g,
// the block's waves are summed into the group-major bcnt[g * nb + b], ONE exclusive scan over its n_groups * nb + 1 elements
// gives every (group, block) its output offset and the per-group counts, and the fill kernel recomputes the predicate.  The
// predicates, their validation and the entry points stay in the two files.
#pragma once

#include "e3_common.h"

namespace e3 {

constexpr int kSelectThreads = 256;
constexpr int kSelectWaves = kSelectThreads / 64;

inline int select_blocks(int64_t n) { return (int)((n + kSelectThreads - 1) / kSelectThreads); }

// n and the group count are in range and every (group, block) offset fits an int32
inline bool select_sizes_ok(int64_t n, int n_groups, int min_groups, int max_groups) {
  return n >= 0 && n_groups >= min_groups && n_groups <= max_groups && n * (int64_t)(n_groups > 0 ? n_groups : 1) < 0x7fffffffLL;
}

// workspace carve-up (bytes, 256-aligned): bcnt | off | scan temp
struct SelectWs {
  size_t bcnt, off, cub, total;
};

inline SelectWs select_ws(int64_t n, int n_groups) {
  const int64_t m = (int64_t)n_groups * select_blocks(n) + 1;
  const size_t arr = ((size_t)m * 4 + 255) / 256 * 256;
  return SelectWs{0, arr, 2 * arr, 2 * arr + (scan_temp_bytes(m) + 255) / 256 * 256};
}

// count kernel, after the barrier that follows its wcnt writes: this block's hits per group
template <int G>
__device__ __forceinline__ void store_block_counts(const int32_t (*wcnt)[G], const int n_groups, int32_t* __restrict__ bcnt) {
  if (threadIdx.x < n_groups) {
    int s = 0;
    for (int w = 0; w < kSelectWaves; ++w) s += wcnt[w][threadIdx.x];
    bcnt[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}

// fill kernel: output slot of this lane's hit in group g; `ballot` = the wave's hits in g, `below` = the lanes before this one
template <int G>
__device__ __forceinline__ int64_t select_slot(const int32_t* __restrict__ off, const int32_t (*wcnt)[G], const int g,
                                               const int wave, const unsigned long long ballot,
                                               const unsigned long long below) {
  int64_t o = off[(int64_t)g * gridDim.x + blockIdx.x] + __popcll(ballot & below);
  for (int w = 0; w < wave; ++w) o += wcnt[w][g];
  return o;
}

// off = exclusive scan of bcnt (n_groups * nb + 1 elements): counts[g] = off[(g + 1) nb] - off[g nb]
static __global__ void select_counts_kernel(const int32_t* __restrict__ off, int nb, int n_groups, int32_t* __restrict__ counts) {
  const int g = threadIdx.x;
  if (g < n_groups) counts[g] = off[(int64_t)(g + 1) * nb] - off[(int64_t)g * nb];
}

// host, count side for n > 0: zero the scan's last input, launch_count(bcnt), scan, per-group counts (no groups: the count
// launch alone)
template <class Launch>
int select_count(void* workspace, const SelectWs& w, int nb, int n_groups, int32_t* counts, hipStream_t s, Launch launch_count) {
  char* ws = static_cast<char*>(workspace);
  int32_t* bcnt = (int32_t*)(ws + w.bcnt);
  int32_t* off = (int32_t*)(ws + w.off);
  const int64_t m = (int64_t)n_groups * nb + 1;
  E3_HIP_CHECK(hipMemsetAsync(bcnt + (m - 1), 0, 4, s));
  launch_count(bcnt);
  if (n_groups > 0) {
    E3_HIP_CHECK(exclusive_sum(ws + w.cub, scan_temp_bytes(m), bcnt, off, m, s));
    hipLaunchKernelGGL(select_counts_kernel, dim3(1), dim3(64), 0, s, off, nb, n_groups, counts);
  }
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // namespace e3
