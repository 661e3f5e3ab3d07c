// Periodic halo: which owned particles go to which ghost image, and where they land (sharding.GridHalo.setup with
// `periodic`).  Spec: include/e3gnn.h, e3_halo_select_count.  Integer / HBM work, no MFMA: one thread per particle loops
// over the (<= 26) entries; a wave counts its hits with one 64-bit ballot per entry, the waves of a block meet in LDS, and
// an exclusive scan over the entry-major [n_entries, n_blocks] block counts gives every (entry, block) its output offset.
// The fill pass recomputes the same predicate, so the output is grouped by entry with ascending particle ids inside a
// group -- the order of mask.nonzero() on an entry-major [n_entries, n] mask.
// The count / scan / fill scaffold is e3_select.h, shared with e3_morton_halo.hip.
#include "e3_select.h"

#include <cmath>

namespace e3 {

// by value as a kernel argument (~1 KiB)
struct HaloDev {
  float lo[3], hi[3], L[3], invL[3];
  int periodic;
  int n_entries;
  float elo[E3_HALO_MAX_ENTRIES][3], ehi[E3_HALO_MAX_ENTRIES][3], esh[E3_HALO_MAX_ENTRIES][3];
};

__device__ __forceinline__ bool in_entry(const float3 p, const HaloDev& h, const int e) {
  return p.x >= h.elo[e][0] && p.x < h.ehi[e][0] && p.y >= h.elo[e][1] && p.y < h.ehi[e][1] && p.z >= h.elo[e][2] &&
         p.z < h.ehi[e][2];
}

// wrapped positions out; per (entry, block) hit counts, entry-major: bcnt[e * nb + b]
__global__ __launch_bounds__(kSelectThreads) void halo_count_kernel(const float* __restrict__ pos, int64_t n, const HaloDev h,
                                                                  float* __restrict__ pos_w, int32_t* __restrict__ bcnt) {
  __shared__ int32_t wcnt[kSelectWaves][E3_HALO_MAX_ENTRIES];
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool live = i < n;
  float3 p = make_float3(0.0f, 0.0f, 0.0f);
  if (live) {
    p = make_float3(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2]);
    if (h.periodic & 1) p.x = wrap_coord(p.x, h.lo[0], h.hi[0], h.L[0], h.invL[0]);
    if (h.periodic & 2) p.y = wrap_coord(p.y, h.lo[1], h.hi[1], h.L[1], h.invL[1]);
    if (h.periodic & 4) p.z = wrap_coord(p.z, h.lo[2], h.hi[2], h.L[2], h.invL[2]);
    pos_w[3 * i + 0] = p.x; pos_w[3 * i + 1] = p.y; pos_w[3 * i + 2] = p.z;
  }
  for (int e = 0; e < h.n_entries; ++e) {
    const unsigned long long m = __ballot(live && in_entry(p, h, e));
    if (lane == 0) wcnt[wave][e] = __popcll(m);
  }
  __syncthreads();
  store_block_counts(wcnt, h.n_entries, bcnt);
}

__global__ __launch_bounds__(kSelectThreads) void halo_fill_kernel(const float* __restrict__ pos_w, int64_t n, const HaloDev h,
                                                                 const int32_t* __restrict__ off, int64_t total,
                                                                 int32_t* __restrict__ idx, float* __restrict__ ghost) {
  __shared__ int32_t wcnt[kSelectWaves][E3_HALO_MAX_ENTRIES];
  const int64_t i = blockIdx.x * (int64_t)kSelectThreads + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool live = i < n;
  const float3 p = live ? make_float3(pos_w[3 * i + 0], pos_w[3 * i + 1], pos_w[3 * i + 2]) : make_float3(0.0f, 0.0f, 0.0f);
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes < this one
  uint32_t hit = 0;                                                        // bit e: inside entry e
  for (int e = 0; e < h.n_entries; ++e) {
    const bool in = live && in_entry(p, h, e);
    const unsigned long long m = __ballot(in);
    if (lane == 0) wcnt[wave][e] = __popcll(m);
    hit |= (in ? 1u : 0u) << e;
  }
  __syncthreads();
  if (!hit) return;   // the ballots below see the exited lanes as 0, which they are
  for (int e = 0; e < h.n_entries; ++e) {
    const bool in = (hit >> e) & 1;
    const unsigned long long m = __ballot(in);
    if (!in) continue;
    const int64_t o = select_slot(off, wcnt, e, wave, m, below);
    if (o >= total) continue;   // only a caller that changed the inputs between the two calls gets here
    idx[o] = (int32_t)i;
    ghost[3 * o + 0] = __fadd_rn(p.x, h.esh[e][0]);
    ghost[3 * o + 1] = __fadd_rn(p.y, h.esh[e][1]);
    ghost[3 * o + 2] = __fadd_rn(p.z, h.esh[e][2]);
  }
}

static bool halo_sizes_ok(int64_t n, int n_entries) { return select_sizes_ok(n, n_entries, 0, E3_HALO_MAX_ENTRIES); }

// host: validated device parameters (finite non-empty bounds, a mask in [0, 7], 2 r < L on periodic axes)
static int halo_dev(const float lo[3], const float hi[3], int periodic, float r, const e3_halo_entry* entries, int n_entries,
                    HaloDev* h) {
  if (!lo || !hi || periodic < 0 || periodic > 7 || n_entries < 0 || n_entries > E3_HALO_MAX_ENTRIES) return E3_ERR_INVALID_ARG;
  if (n_entries > 0 && !entries) return E3_ERR_INVALID_ARG;
  if (!std::isfinite(r) || r < 0.0f) return E3_ERR_INVALID_ARG;
  *h = HaloDev{};
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(lo[a] < hi[a])) return E3_ERR_INVALID_ARG;
    const float L = hi[a] - lo[a];
    const bool on = (periodic >> a) & 1;
    if (on && !(std::isfinite(L) && 2.0f * r < L)) return E3_ERR_INVALID_ARG;
    h->lo[a] = lo[a];
    h->hi[a] = hi[a];
    h->L[a] = on ? L : 0.0f;
    h->invL[a] = on ? 1.0f / L : 0.0f;
  }
  h->periodic = periodic;
  h->n_entries = n_entries;
  for (int e = 0; e < n_entries; ++e)
    for (int a = 0; a < 3; ++a) {
      const float l = entries[e].lo[a], u = entries[e].hi[a], s = entries[e].shift[a];
      if (std::isnan(l) || std::isnan(u) || !std::isfinite(s)) return E3_ERR_INVALID_ARG;
      h->elo[e][a] = l;
      h->ehi[e][a] = u;
      h->esh[e][a] = s;
    }
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int64_t e3_halo_select_workspace_bytes(int64_t n, int n_entries) {
  if (!halo_sizes_ok(n, n_entries)) return -1;
  return (int64_t)select_ws(n, n_entries).total;
}

int e3_halo_select_count(const float* pos, int64_t n, const float lo[3], const float hi[3], int32_t periodic, float r,
                         const e3_halo_entry* entries, int n_entries, float* pos_wrapped, int32_t* counts, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  if (!halo_sizes_ok(n, n_entries)) return E3_ERR_INVALID_ARG;
  HaloDev h;
  const int st = halo_dev(lo, hi, periodic, r, entries, n_entries, &h);
  if (st != E3_OK) return st;
  if ((n > 0 && (!pos || !pos_wrapped)) || (n_entries > 0 && !counts) || !workspace) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_entries);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (n_entries > 0) E3_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_entries * 4, s));
    return E3_OK;
  }
  const int nb = select_blocks(n);
  return select_count(workspace, w, nb, n_entries, counts, s, [&](int32_t* bcnt) {   // no entries: the wrap alone
    hipLaunchKernelGGL(halo_count_kernel, dim3(nb), dim3(kSelectThreads), 0, s, pos, n, h, pos_wrapped, bcnt);
  });
}

int e3_halo_select_fill(const float* pos_wrapped, int64_t n, const float lo[3], const float hi[3], int32_t periodic, float r,
                        const e3_halo_entry* entries, int n_entries, int64_t total, int32_t* idx, float* ghost_pos,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  if (!halo_sizes_ok(n, n_entries)) return E3_ERR_INVALID_ARG;
  HaloDev h;
  const int st = halo_dev(lo, hi, periodic, r, entries, n_entries, &h);
  if (st != E3_OK) return st;
  if (total < 0) return E3_ERR_INVALID_ARG;
  if (n == 0 || n_entries == 0 || total == 0) return E3_OK;
  if (!pos_wrapped || !idx || !ghost_pos || !workspace) return E3_ERR_INVALID_ARG;
  const SelectWs w = select_ws(n, n_entries);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(halo_fill_kernel, dim3(select_blocks(n)), dim3(kSelectThreads), 0, s, pos_wrapped, n, h,
                     (const int32_t*)(static_cast<char*>(workspace) + w.off), total, idx, ghost_pos);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // extern "C"
