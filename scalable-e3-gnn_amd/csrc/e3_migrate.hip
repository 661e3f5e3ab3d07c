// Particle migration between ranks (sharding.Halo.migrate): the rows of an int32 row table [n, W] are split by a given
// owner[n] into `stay` (owner == self_rank, original order) and `send` (the others, grouped by destination rank ascending,
// ascending row ids inside a group).  Spec: include/e3gnn.h, e3_migrate_count.  Integer / HBM work, no MFMA.  Ownership is an
// INPUT: the rule lives in halo.owner_of alone, nothing here recomputes it.
//
// Counting and placement are e3_select.h's, group = destination rank (the stayers are group self_rank): one thread per row,
// per wave a loop over the destinations PRESENT in it -- the first unretired lane's owner, one 64-bit ballot of the lanes
// that share it, popcount, retire them; most rows stay, so one to three turns is the rule and 64 the worst case -- the waves
// of a block summed in LDS into the rank-major bcnt[q * nb + b], one exclusive scan.  A row whose owner lies outside
// [0, n_ranks) joins no group: it is counted as n - (the scan's total) and nothing is ever indexed by its owner.  The fill
// pass recomputes the ballots, so a row's slot is (group, block) offset + waves before + lanes before: plain stores, a fixed
// order, no atomics.  Rows are copied by lane groups of L = the power of two >= min(W, 64) lanes, 64 / L rows per pass, each
// lane striding over the row's words: consecutive lanes read and write consecutive dwords.
#include "e3_select.h"

namespace e3 {

constexpr int kMigrateMaxWords = 4096;

// this lane's group: owner[i] inside [0, n_ranks), else -1 (past the end, or an invalid owner)
__device__ __forceinline__ int migrate_group(const int32_t* __restrict__ owner, const int64_t n, const int n_ranks) {
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  if (i >= n) return -1;
  const int o = owner[i];
  return (o >= 0 && o < n_ranks) ? o : -1;
}

// wcnt[wave][q] = the number of lanes of each wave in group q, zero for the groups absent from the wave; returns, for a
// lane with a group, the ballot of its group's lanes (0 otherwise).  Every thread of the block calls it.
__device__ __forceinline__ unsigned long long migrate_wave_groups(const int g, int32_t (*__restrict__ wcnt)[E3_MORTON_MAX_RANKS]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  wcnt[wave][lane] = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (unsigned long long left = __ballot(g >= 0); left;) {
    const int q = __builtin_amdgcn_readfirstlane(__shfl(g, (int)__builtin_ctzll(left)));
    const unsigned long long b = __ballot(g == q);
    if (g == q) mine = b;
    if (lane == 0) wcnt[wave][q] = __popcll(b);
    left &= ~b;
  }
  __syncthreads();
  return mine;
}

__global__ __launch_bounds__(kSelectThreads) void migrate_count_kernel(const int32_t* __restrict__ owner, int64_t n, int n_ranks,
                                                                       int32_t* __restrict__ bcnt) {
  __shared__ int32_t wcnt[kSelectWaves][E3_MORTON_MAX_RANKS];
  migrate_wave_groups(migrate_group(owner, n, n_ranks), wcnt);
  store_block_counts(wcnt, n_ranks, bcnt);
}

// counts[n_ranks] = the rows in no group; off[n_ranks * nb] = the scan's total
static __global__ void migrate_invalid_kernel(const int32_t* __restrict__ off, int64_t last, int64_t n, int32_t* __restrict__ out) {
  if (threadIdx.x == 0) *out = (int32_t)(n - off[last]);
}

__global__ __launch_bounds__(kSelectThreads) void migrate_fill_kernel(const int32_t* __restrict__ table,
                                                                      const int32_t* __restrict__ owner, int64_t n, int W,
                                                                      int log2L, int n_ranks, int self,
                                                                      const int32_t* __restrict__ off, int64_t stay_rows,
                                                                      int64_t send_rows, int32_t* __restrict__ stay,
                                                                      int32_t* __restrict__ send) {
  __shared__ int32_t wcnt[kSelectWaves][E3_MORTON_MAX_RANKS];
  const int g = migrate_group(owner, n, n_ranks);
  const unsigned long long b = migrate_wave_groups(g, wcnt);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes < this one
  // the row's slot in its output, -1 = no copy.  off is the scan over ALL groups, the stayers' among them: a stayer's slot
  // is relative to the start of group self, a leaver's skips that group when its destination comes after it.  A slot at or
  // past its capacity is reached only by a caller that changed owner[] between the two calls.
  int slot = -1;
  const int to_stay = g == self;
  if (g >= 0) {
    const int64_t nb = gridDim.x;
    int64_t o = select_slot(off, wcnt, g, wave, b, below);
    if (g >= self) o -= g == self ? off[(int64_t)self * nb] : off[(int64_t)(self + 1) * nb] - off[(int64_t)self * nb];
    if (o >= 0 && o < (to_stay ? stay_rows : send_rows)) slot = (int)o;
  }
  // the wave copies its 64 rows: lane group `sub` takes row pass * rows_per_pass + sub, lane w0 of it the words w0, w0 + L, ..
  const int L = 1 << log2L, per_pass = 64 >> log2L;
  const int sub = lane >> log2L, w0 = lane & (L - 1);
  const int64_t row0 = blockIdx.x * (int64_t)kSelectThreads + wave * 64;
  for (int pass = 0; pass < L; ++pass) {
    const int r = pass * per_pass + sub;
    const int s = __shfl(slot, r), st = __shfl(to_stay, r);
    if (s < 0) continue;
    const int32_t* __restrict__ from = table + (row0 + r) * W;
    int32_t* __restrict__ to = (st ? stay : send) + (int64_t)s * W;
    for (int w = w0; w < W; w += L) to[w] = from[w];
  }
}

static bool migrate_sizes_ok(int64_t n, int n_ranks) { return select_sizes_ok(n, n_ranks, 1, E3_MORTON_MAX_RANKS); }

}  // namespace e3

using namespace e3;

extern "C" {

int64_t e3_migrate_workspace_bytes(int64_t n, int n_ranks) {
  if (!migrate_sizes_ok(n, n_ranks)) return -1;
  return (int64_t)select_ws(n, n_ranks).total;
}

int e3_migrate_count(const int32_t* owner, int64_t n, int n_ranks, int self_rank, int32_t* counts, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (!migrate_sizes_ok(n, n_ranks) || self_rank < 0 || self_rank >= n_ranks) return E3_ERR_INVALID_ARG;
  if ((n > 0 && !owner) || !counts || !workspace) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_ranks);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    E3_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(n_ranks + 1) * 4, s));
    return E3_OK;
  }
  const int nb = select_blocks(n);
  const int st = select_count(workspace, w, nb, n_ranks, counts, s, [&](int32_t* bcnt) {
    hipLaunchKernelGGL(migrate_count_kernel, dim3(nb), dim3(kSelectThreads), 0, s, owner, n, n_ranks, bcnt);
  });
  if (st != E3_OK) return st;
  hipLaunchKernelGGL(migrate_invalid_kernel, dim3(1), dim3(64), 0, s,
                     (const int32_t*)(static_cast<char*>(workspace) + w.off), (int64_t)n_ranks * nb, n, counts + n_ranks);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_migrate_fill(const int32_t* table, const int32_t* owner, int64_t n, int W, int n_ranks, int self_rank,
                    const int32_t* counts, int64_t stay_rows, int64_t send_rows, int32_t* stay, int32_t* send, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  if (!migrate_sizes_ok(n, n_ranks) || self_rank < 0 || self_rank >= n_ranks) return E3_ERR_INVALID_ARG;
  if (W < 1 || W > kMigrateMaxWords || n * (int64_t)W >= 0x7fffffffLL) return E3_ERR_INVALID_ARG;
  if (!counts || stay_rows < 0 || send_rows < 0) return E3_ERR_INVALID_ARG;
  // the counts the caller read: every row is in exactly one of them, and each output holds what they say
  int64_t total = 0;
  for (int q = 0; q <= n_ranks; ++q) {
    if (counts[q] < 0) return E3_ERR_INVALID_ARG;
    total += counts[q];
  }
  const int64_t n_stay = counts[self_rank], n_send = total - n_stay - counts[n_ranks];
  if (total != n || n_stay > stay_rows || n_send > send_rows) return E3_ERR_INVALID_ARG;
  if (n == 0 || n_stay + n_send == 0) return E3_OK;
  if (!table || !owner || !workspace || (n_stay > 0 && !stay) || (n_send > 0 && !send)) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_ranks);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  int log2L = 0;
  while (log2L < 6 && (1 << log2L) < W) ++log2L;
  hipLaunchKernelGGL(migrate_fill_kernel, dim3(select_blocks(n)), dim3(kSelectThreads), 0, (hipStream_t)stream, table, owner, n,
                     W, log2L, n_ranks, self_rank, (const int32_t*)(static_cast<char*>(workspace) + w.off), n_stay, n_send,
                     stay, send);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
