// Radius graph on the GPU: Morton keys -> stable radix sort -> cell table -> per-cell LDS-staged
// neighbour scan, emitting CSR-by-dst with ascending src.  Spec: include/e3gnn.h (builder-defined,
// SURVEY.md §8a-N1).  All edge decisions use explicitly rounded fp32 operations (no FMA contraction)
// so that the CPU oracle reproduces them bit for bit.
#include "e3_common.h"

#include <hipcub/hipcub.hpp>   // DeviceRadixSort; the scan is e3_scan.hip's

#include <algorithm>
#include <cmath>

namespace e3 {

constexpr int kCandCap = 1024;  // candidates staged per chunk (16 KiB of LDS per wave)

__host__ __device__ inline uint32_t compact3(uint32_t v) {
  v &= 0x09249249;
  v = (v | (v >> 2)) & 0x030C30C3;
  v = (v | (v >> 4)) & 0x0300F00F;
  v = (v | (v >> 8)) & 0x030000FF;
  v = (v | (v >> 16)) & 0x3ff;
  return v;
}
struct RgDev {
  float lo[3], inv[3];
  int n[3];
  float r2;
  int bits;
};

// periodic axes (the *_pbc entries; include/e3gnn.h): box length L = hi - lo, 1 / L, hL = L / 2 (+inf on an open axis: the
// edge-test shift never fires there), bit a of `periodic` = axis a
struct RgPbc {
  float hi[3], L[3], invL[3], hL[3];
  int periodic;
};

// general cell (the *_cell entries): RgCell, cell_s and wrap_cell are in e3_common.h, shared with e3_cell_images.hip
// the periodic argument of a mode's kernels (the open kernels carry an unread RgPbc)
template <int MODE> struct RgArg { using type = RgPbc; };
template <> struct RgArg<kCell> { using type = RgCell; };

template <int PBC>
__device__ __forceinline__ float3 load_pos(const float* __restrict__ pos, const int64_t o, const RgDev& g,
                                           const typename RgArg<PBC>::type& pb) {
  float3 p = make_float3(pos[3 * o + 0], pos[3 * o + 1], pos[3 * o + 2]);
  if constexpr (PBC == kCell) {
    p = wrap_cell(pb, p);
  } else if constexpr (PBC == kBox) {
    if (pb.periodic & 1) p.x = wrap_coord(p.x, g.lo[0], pb.hi[0], pb.L[0], pb.invL[0]);
    if (pb.periodic & 2) p.y = wrap_coord(p.y, g.lo[1], pb.hi[1], pb.L[1], pb.invL[1]);
    if (pb.periodic & 4) p.z = wrap_coord(p.z, g.lo[2], pb.hi[2], pb.L[2], pb.invL[2]);
  }
  return p;
}

template <int PBC>
__global__ void rg_keys_kernel(const float* __restrict__ pos, int64_t N, RgDev g, uint32_t* __restrict__ keys,
                               int32_t* __restrict__ idx, const typename RgArg<PBC>::type pb) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  float3 p = load_pos<PBC>(pos, i, g, pb);
  if constexpr (PBC == kCell) {  // the grid coordinate q_a = s_a(w) h_a
    float s[3];
    cell_s(pb, p, s);
    p = make_float3(__fmul_rn(s[0], pb.hgt[0]), __fmul_rn(s[1], pb.hgt[1]), __fmul_rn(s[2], pb.hgt[2]));
  }
  int cx = cell_of(p.x, g.lo[0], g.inv[0], g.n[0]);
  int cy = cell_of(p.y, g.lo[1], g.inv[1], g.n[1]);
  int cz = cell_of(p.z, g.lo[2], g.inv[2], g.n[2]);
  keys[i] = morton3(cx, cy, cz);
  idx[i] = (int32_t)i;
}

// sorted positions (x,y,z,0; PBC: wrapped), cell table [begin,end) per Morton code, list of non-empty cells
template <int PBC>
__global__ void rg_cells_kernel(const float* __restrict__ pos, int64_t N, const uint32_t* __restrict__ skeys,
                                const int32_t* __restrict__ perm, float4* __restrict__ spos,
                                int32_t* __restrict__ cbegin, int32_t* __restrict__ cend,
                                int32_t* __restrict__ heads, int32_t* __restrict__ nheads, const RgDev g,
                                const typename RgArg<PBC>::type pb) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t o = perm[i];
  if constexpr (PBC != kOpen) {
    const float3 p = load_pos<PBC>(pos, o, g, pb);
    spos[i] = make_float4(p.x, p.y, p.z, 0.0f);
  } else {
    spos[i] = make_float4(pos[3 * (int64_t)o], pos[3 * (int64_t)o + 1], pos[3 * (int64_t)o + 2], 0.0f);
  }
  const uint32_t k = skeys[i];
  if (i == 0 || skeys[i - 1] != k) {
    cbegin[k] = (int32_t)i;
    heads[atomicAdd(nheads, 1)] = (int32_t)i;
  }
  if (i == N - 1 || skeys[i + 1] != k) cend[k] = (int32_t)(i + 1);
}

// The pieces below are shared by the two per-cell kernels (rg_scan_kernel: count and plain fill; rg_nearest_kernel: the
// capped fill), so that both see the same candidates in the same order and take the same edge decisions.
//
// Neighbour table of the cell `code`, by one wave: the id ranges [rb, re) of its (up to 27) non-empty neighbour cells ordered
// by Morton code (=> candidate ids ascend) and their running candidate count pre[0..27].  Returns `shift`: some candidate
// may sit across a periodic face (wave-uniform).
template <int PBC>
__device__ __forceinline__ bool rg_neighbour_table(const uint32_t code, const int lane, const RgDev& g,
                                                   const typename RgArg<PBC>::type& pb,
                                                   const int32_t* __restrict__ cbegin, const int32_t* __restrict__ cend,
                                                   int (&rb)[28], int (&re)[28], int (&pre)[29]) {
  const int cx = (int)compact3(code), cy = (int)compact3(code >> 1), cz = (int)compact3(code >> 2);
  uint32_t ncode = 0xFFFFFFFFu;
  int b = 0, e = 0;
  if (lane < 27) {
    int dx = lane % 3 - 1, dy = (lane / 3) % 3 - 1, dz = lane / 9 - 1;
    int x = cx + dx, y = cy + dy, z = cz + dz;
    if constexpr (PBC == kCell) {
      x = x < 0 ? x + g.n[0] : (x >= g.n[0] ? x - g.n[0] : x);
      y = y < 0 ? y + g.n[1] : (y >= g.n[1] ? y - g.n[1] : y);
      z = z < 0 ? z + g.n[2] : (z >= g.n[2] ? z - g.n[2] : z);
    } else if constexpr (PBC == kBox) {
      if (pb.periodic & 1) x = x < 0 ? x + g.n[0] : (x >= g.n[0] ? x - g.n[0] : x);
      if (pb.periodic & 2) y = y < 0 ? y + g.n[1] : (y >= g.n[1] ? y - g.n[1] : y);
      if (pb.periodic & 4) z = z < 0 ? z + g.n[2] : (z >= g.n[2] ? z - g.n[2] : z);
    }
    if (x >= 0 && x < g.n[0] && y >= 0 && y < g.n[1] && z >= 0 && z < g.n[2]) {
      ncode = morton3(x, y, z);
      b = cbegin[ncode];
      e = cend[ncode];
      if (e <= b) ncode = 0xFFFFFFFFu;  // empty
    }
  }
  bool shift = false;
  if constexpr (PBC != kOpen) {
    bool dup = false;  // the same cell under a lower offset (n <= 2 on a periodic axis)
    for (int m = 0; m < 27; ++m) dup |= (__shfl(ncode, m) == ncode) && (m < lane);
    if (dup) ncode = 0xFFFFFFFFu;
    // n >= 5 and a cell away from both faces: |x_i - x_j| < 2 cell widths + rounding < L / 2, the shift never fires
    const int c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; ++a) {
      bool on = true;
      if constexpr (PBC == kBox) on = (pb.periodic >> a) & 1;
      if (on) shift |= g.n[a] < 5 || c[a] < 1 || c[a] > g.n[a] - 2;
    }
  }
  int rank = 0;
  for (int m = 0; m < 27; ++m) {
    uint32_t other = __shfl(ncode, m);
    rank += (other < ncode) || (other == ncode && m < lane);
  }
  if (lane < 27) {
    rb[rank] = (ncode == 0xFFFFFFFFu) ? 0 : b;
    re[rank] = (ncode == 0xFFFFFFFFu) ? 0 : e;
  }
  __syncthreads();
  if (lane == 0) {
    int acc = 0;
    for (int m = 0; m < 27; ++m) { pre[m] = acc; acc += re[m] - rb[m]; }
    pre[27] = acc;
  }
  __syncthreads();
  return shift;
}

// candidates [c0, c0 + nc) of the table into LDS: x, y, z and the id (bit pattern)
__device__ __forceinline__ void rg_stage(const float4* __restrict__ spos, const int lane, const int c0, const int nc,
                                         const int (&rb)[28], const int (&pre)[29], float4 (&cand)[kCandCap]) {
  for (int f = lane; f < nc; f += 64) {
    const int ff = c0 + f;
    int m = 0;
    while (ff >= pre[m + 1]) ++m;
    const int gid = rb[m] + (ff - pre[m]);
    float4 p = spos[gid];
    p.w = __int_as_float(gid);
    cand[f] = p;
  }
  __syncthreads();
}

// d2 of the edge test (include/e3gnn.h): x_i - x_j, its image shift where `shift` says a face may lie between them, and the
// explicitly rounded sum of squares.  The ONE statement of it: the count pass, the plain fill, the capped fill and the keys
// the capped fill orders by all come from here.
template <int PBC>
__device__ __forceinline__ float rg_d2(const float4 pi, const float4 pc, const bool shift,
                                       const typename RgArg<PBC>::type& pb) {
  float dx = __fsub_rn(pi.x, pc.x), dy = __fsub_rn(pi.y, pc.y), dz = __fsub_rn(pi.z, pc.z);
  if constexpr (PBC == kCell) {
    if (shift) min_image(pb.c, dx, dy, dz);
  } else if (PBC == kBox && shift) {
    dx = dx > pb.hL[0] ? __fsub_rn(dx, pb.L[0]) : (dx < -pb.hL[0] ? __fadd_rn(dx, pb.L[0]) : dx);
    dy = dy > pb.hL[1] ? __fsub_rn(dy, pb.L[1]) : (dy < -pb.hL[1] ? __fadd_rn(dy, pb.L[1]) : dy);
    dz = dz > pb.hL[2] ? __fsub_rn(dz, pb.L[2]) : (dz < -pb.hL[2] ? __fadd_rn(dz, pb.L[2]) : dz);
  }
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// One wave per non-empty cell.  FILL=false: deg[i] = #neighbours.  FILL=true: src[rowptr[i]..] = ids.
// PBC: neighbour cells modulo n on periodic axes (duplicates dropped: n <= 2 names a cell more than once) and the one-step
// minimum image in the edge test -- skipped by the cells whose 3x3x3 neighbourhood stays inside the box (wave-uniform).
// kCell: the same on the grid of q (every direction periodic), with the rint minimum image of the cell in the edge test.
template <bool FILL, int PBC>
__global__ __launch_bounds__(64) void rg_scan_kernel(const float4* __restrict__ spos, const uint32_t* __restrict__ skeys,
                                                     const int32_t* __restrict__ cbegin,
                                                     const int32_t* __restrict__ cend,
                                                     const int32_t* __restrict__ heads,
                                                     const int32_t* __restrict__ nheads_p, RgDev g,
                                                     int32_t* __restrict__ deg, const int32_t* __restrict__ rowptr,
                                                     int32_t* __restrict__ src,
                                                     const typename RgArg<PBC>::type pb) {
  __shared__ float4 cand[kCandCap];   // x,y,z, id (bit pattern)
  __shared__ int rb[28], re[28], pre[29];
  const int lane = threadIdx.x;
  const int nheads = *nheads_p;
  for (int h = blockIdx.x; h < nheads; h += gridDim.x) {
    const int cb = heads[h];
    const uint32_t code = skeys[cb];
    const int ce = cend[code];
    const bool shift = rg_neighbour_table<PBC>(code, lane, g, pb, cbegin, cend, rb, re, pre);
    const int ncand = pre[27];
    for (int c0 = 0; c0 < ncand; c0 += kCandCap) {
      const int nc = min(kCandCap, ncand - c0);
      rg_stage(spos, lane, c0, nc, rb, pre, cand);
      for (int i = cb; i < ce; ++i) {
        const float4 pi = spos[i];
        int cnt = 0;
        // deg[] carries the running per-row count between candidate chunks (only when ncand > kCandCap);
        // agent-scope atomics keep that hand-over out of the per-CU L1.
        const int prev = (c0 > 0) ? __hip_atomic_load(&deg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const int cursor = FILL ? (rowptr[i] + prev) : 0;
        for (int base = 0; base < nc; base += 64) {
          const int c = base + lane;
          bool ok = false;
          int id = -1;
          if (c < nc) {
            const float4 pc = cand[c];
            id = __float_as_int(pc.w);
            ok = (id != i) && (rg_d2<PBC>(pi, pc, shift, pb) <= g.r2);
          }
          const unsigned long long mask = __ballot(ok);
          if (FILL && ok) src[cursor + cnt + __popcll(mask & ((1ull << lane) - 1ull))] = id;
          cnt += __popcll(mask);
        }
        if (lane == 0 && (!FILL || c0 + kCandCap < ncand))
          __hip_atomic_store(&deg[i], prev + cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
  }
}

// ---- capped rows: the k nearest inside r (include/e3gnn.h, e3_rg_fill_nearest) ----------------------------------------
// A candidate's key is (d2 bits << 32) | id: d2 >= 0, so its bit pattern orders as its value, and the id breaks ties towards
// the lower one.  A rejected candidate (outside r, the row itself, past the end of the chunk) carries the all-ones key, which
// no accepted candidate reaches (an id is below 2^31).
using rg_key_t = unsigned long long;
constexpr rg_key_t kNoKey = ~0ull;
__device__ __forceinline__ rg_key_t rg_key(const float d2, const int id) {
  return ((rg_key_t)__float_as_uint(d2) << 32) | (uint32_t)id;
}
// compare-exchange with lane ^ j: this lane keeps the smaller of the two when `low`
__device__ __forceinline__ rg_key_t rg_cmpx(const rg_key_t v, const int j, const bool low) {
  const rg_key_t o = __shfl_xor(v, j);
  return (o < v) == low ? o : v;
}
// a bitonic sequence across the wave -> ascending with the lane (6 steps)
__device__ __forceinline__ rg_key_t rg_wave_merge(rg_key_t v, const int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) v = rg_cmpx(v, j, (lane & j) == 0);
  return v;
}
// any 64 keys across the wave -> ascending with the lane (bitonic, 21 steps)
__device__ __forceinline__ rg_key_t rg_wave_sort(rg_key_t v, const int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) v = rg_cmpx(v, j, ((lane & k) == 0) == ((lane & j) == 0));
  return v;
}

// The fill of a capped graph: rg_scan_kernel<true> with rowptr = the scan of min(deg, k).  deg[i] is the full degree the count
// pass left; cursor[] carries a plain row's fill position between candidate chunks.  A row with deg <= k takes the plain
// ballot / popcount path.  A row above k keeps its best k keys sorted across the lanes: a batch of 64 candidates that holds
// nothing below the current k-th key is skipped; otherwise the batch is sorted, reversed and merged (the lane-wise minimum of
// an ascending and a descending run is bitonic and holds the 64 smallest of the 128).  Between chunks such a row parks its
// ids in its own k slots of src (-1 = none yet) and recomputes their keys from the positions when it resumes: the same
// expression on the same operands, so the same bits.  Every store is bounded by the row's capacity rowptr[i + 1] - rowptr[i].
template <int PBC>
__global__ __launch_bounds__(64) void rg_nearest_kernel(const float4* __restrict__ spos, const uint32_t* __restrict__ skeys,
                                                        const int32_t* __restrict__ cbegin,
                                                        const int32_t* __restrict__ cend,
                                                        const int32_t* __restrict__ heads,
                                                        const int32_t* __restrict__ nheads_p, RgDev g,
                                                        const int32_t* __restrict__ deg, int32_t* __restrict__ cursor,
                                                        const int32_t* __restrict__ rowptr, int32_t* src, const int k,
                                                        const typename RgArg<PBC>::type pb) {
  __shared__ float4 cand[kCandCap];
  __shared__ int rb[28], re[28], pre[29];
  const int lane = threadIdx.x;
  const int nheads = *nheads_p;
  for (int h = blockIdx.x; h < nheads; h += gridDim.x) {
    const int cb = heads[h];
    const uint32_t code = skeys[cb];
    const int ce = cend[code];
    const bool shift = rg_neighbour_table<PBC>(code, lane, g, pb, cbegin, cend, rb, re, pre);
    const int ncand = pre[27];
    for (int c0 = 0; c0 < ncand; c0 += kCandCap) {
      const int nc = min(kCandCap, ncand - c0);
      const bool first = c0 == 0, last = c0 + kCandCap >= ncand;
      rg_stage(spos, lane, c0, nc, rb, pre, cand);
      for (int i = cb; i < ce; ++i) {
        const float4 pi = spos[i];
        const int row = rowptr[i];
        const int cap = min(rowptr[i + 1] - row, k);  // the slots this row owns
        if (deg[i] <= k) {
          // agent-scope atomics keep the hand-over between chunks out of the per-CU L1, as in rg_scan_kernel
          const int prev = first ? 0 : __hip_atomic_load(&cursor[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int cnt = prev;
          for (int base = 0; base < nc; base += 64) {
            const int c = base + lane;
            bool ok = false;
            int id = -1;
            if (c < nc) {
              const float4 pc = cand[c];
              id = __float_as_int(pc.w);
              ok = (id != i) && (rg_d2<PBC>(pi, pc, shift, pb) <= g.r2);
            }
            const unsigned long long mask = __ballot(ok);
            const int at = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (ok && at < cap) src[row + at] = id;
            cnt += __popcll(mask);
          }
          if (lane == 0 && !last) __hip_atomic_store(&cursor[i], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          rg_key_t kept = kNoKey;  // ascending with the lane; lanes [0, k) are the row so far
          if (!first && lane < cap) {
            const int id = __hip_atomic_load(&src[row + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (id >= 0) kept = rg_key(rg_d2<PBC>(pi, spos[id], shift, pb), id);
          }
          rg_key_t worst = __shfl(kept, k - 1);
          for (int base = 0; base < nc; base += 64) {
            const int c = base + lane;
            rg_key_t key = kNoKey;
            if (c < nc) {
              const float4 pc = cand[c];
              const int id = __float_as_int(pc.w);
              const float d2 = rg_d2<PBC>(pi, pc, shift, pb);
              if ((id != i) && (d2 <= g.r2)) key = rg_key(d2, id);
            }
            if (__ballot(key < worst) == 0ull) continue;
            key = rg_wave_sort(key, lane);
            const rg_key_t rev = __shfl(key, 63 - lane);
            kept = rg_wave_merge(rev < kept ? rev : kept, lane);
            worst = __shfl(kept, k - 1);
          }
          if (!last) {
            if (lane < cap) __hip_atomic_store(&src[row + lane], (int)(uint32_t)kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            const rg_key_t ids = rg_wave_sort(lane < k ? (kept & 0xFFFFFFFFull) : kNoKey, lane);
            if (lane < cap) src[row + lane] = (int)(uint32_t)ids;
          }
        }
      }
      __syncthreads();
    }
  }
}

// rowptr_full -> the capped degrees min(deg, k) (and 0 at N, the scan's last input), the number of rows above k and the full
// edge count in 64 bits.  deg is the wrapping int32 difference: below 2^31 even when the running sum has wrapped.
// Grid-stride over at most kCapBlocks blocks with ONE pair of atomics per block: a pair per wave of a flat launch serialises
// 2 x 15 k atomics on two addresses at 1 M rows (190 us measured, against some 10 us of memory traffic).
constexpr int kCapBlocks = 1024;
__global__ __launch_bounds__(256) void rg_cap_kernel(const int32_t* __restrict__ rowptr_full, const int64_t N, const int k,
                                                     int32_t* __restrict__ capdeg, unsigned long long* __restrict__ stats) {
  __shared__ long long sfull[4];
  __shared__ int scut[4];
  long long full = 0;
  int ncut = 0;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i <= N; i += gridDim.x * 256ll) {
    if (i < N) {
      const int d = (int)((uint32_t)rowptr_full[i + 1] - (uint32_t)rowptr_full[i]);
      capdeg[i] = d < 0 ? 0 : min(d, k);
      full += d < 0 ? 0 : d;
      ncut += d > k;
    } else {
      capdeg[N] = 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    full += __shfl_down(full, o);
    ncut += __shfl_down(ncut, o);
  }
  if ((threadIdx.x & 63) == 0) {
    sfull[threadIdx.x >> 6] = full;
    scut[threadIdx.x >> 6] = ncut;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    full = (sfull[0] + sfull[1]) + (sfull[2] + sfull[3]);
    ncut = (scut[0] + scut[1]) + (scut[2] + scut[3]);
    if (ncut) atomicAdd(&stats[0], (unsigned long long)ncut);
    if (full) atomicAdd(&stats[1], (unsigned long long)full);
  }
}

struct RgWs {  // workspace carve-up (bytes, 256-aligned)
  size_t keys, skeys, idx, cbegin, cend, heads, nheads, deg, cub, cub_bytes, total;
};
static RgWs rg_ws(int64_t N, int bits) {
  RgWs w;
  size_t pos = 0;
  auto take = [&](size_t bytes) { size_t o = pos; pos += (bytes + 255) / 256 * 256; return o; };
  size_t ncode = (size_t)1 << (3 * bits);
  w.keys = take(N * 4); w.skeys = take((N + 1) * 4); w.idx = take(N * 4);
  w.cbegin = take(ncode * 4); w.cend = take(ncode * 4);
  w.heads = take(N * 4); w.nheads = take(256); w.deg = take((N + 1) * 4);
  size_t s1 = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, s1, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                     (int32_t*)nullptr, (int)N, 0, 3 * bits);
  w.cub_bytes = std::max(s1, scan_temp_bytes(N + 1)) + 256;
  w.cub = take(w.cub_bytes);
  w.total = pos;
  return w;
}

static RgDev rg_dev(const e3_rg_params* p) {
  RgDev g;
  for (int a = 0; a < 3; ++a) { g.lo[a] = p->lo[a]; g.inv[a] = p->inv[a]; g.n[a] = p->n[a]; }
  g.r2 = p->r * p->r;  // fp32 product
  g.bits = p->bits;
  return g;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_rg_grid(e3_rg_params* p) {
  if (!p || !(p->r > 0.0f)) return E3_ERR_INVALID_ARG;
  int nmax = 1;
  for (int a = 0; a < 3; ++a) {
    float ext = p->hi[a] - p->lo[a];
    if (!(ext > 0.0f)) return E3_ERR_INVALID_ARG;
    float q = floorf(ext / (p->r * 1.0001f));
    int n = q < 1.0f ? 1 : (q > 256.0f ? 256 : (int)q);
    p->n[a] = n;
    p->inv[a] = (float)n / ext;
    nmax = std::max(nmax, n);
  }
  int bits = 1;
  while ((1 << bits) < nmax) ++bits;
  p->bits = bits;
  return E3_OK;
}

int64_t e3_rg_workspace_bytes(int64_t N, const e3_rg_params* p) {
  if (!p || N < 0 || N >= (1ll << 31) - 2 || p->bits < 1 || p->bits > 8) return -1;
  return (int64_t)rg_ws(N, p->bits).total;
}

}  // extern "C"

// host: the device box of a periodic mask (validated: 2 r < L = hi - lo on every periodic axis)
static int rg_pbc(const e3_rg_params* p, int periodic, RgPbc* pb) {
  if (!p || periodic < 0 || periodic > 7) return E3_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a) {
    const float L = p->hi[a] - p->lo[a];
    const bool on = (periodic >> a) & 1;
    if (on && !(L > 0.0f && 2.0f * p->r < L && L < 3.0e38f)) return E3_ERR_INVALID_ARG;
    pb->hi[a] = p->hi[a];
    pb->L[a] = on ? L : 0.0f;
    pb->invL[a] = on ? 1.0f / L : 0.0f;
    pb->hL[a] = on ? 0.5f * L : INFINITY;
  }
  pb->periodic = periodic;
  return E3_OK;
}

// host: the device cell of a *_cell entry (validated: a derivable cell, finite origin, 2 r < every height, and prm = the grid
// of e3_rg_grid over lo = 0, hi = the heights)
static int rg_cell(const e3_rg_params* p, const float* cell, const float* origin, RgCell* rc) {
  if (!p || !cell || !origin || !make_cell(cell, p->r, &rc->c, rc->hgt)) return E3_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a) {
    if (!(fabsf(origin[a]) < 3.0e38f) || p->lo[a] != 0.0f || p->hi[a] != rc->hgt[a]) return E3_ERR_INVALID_ARG;
    rc->o[a] = origin[a];
  }
  return E3_OK;
}

template <int PBC>
static int rg_sort_count(const float* pos, int64_t N, const e3_rg_params* p, const typename RgArg<PBC>::type& pb,
                         int32_t* perm, float* sorted_pos4, int32_t* rowptr, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  if (!p || N < 0 || !rowptr || p->bits < 1 || p->bits > 8) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) { E3_HIP_CHECK(hipMemsetAsync(rowptr, 0, 4, s)); return E3_OK; }
  if (!pos || !perm || !sorted_pos4 || !workspace) return E3_ERR_INVALID_ARG;
  RgWs w = rg_ws(N, p->bits);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  char* ws = (char*)workspace;
  RgDev g = rg_dev(p);
  uint32_t* keys = (uint32_t*)(ws + w.keys);
  uint32_t* skeys = (uint32_t*)(ws + w.skeys);
  int32_t* idx = (int32_t*)(ws + w.idx);
  int32_t* cbegin = (int32_t*)(ws + w.cbegin);
  int32_t* cend = (int32_t*)(ws + w.cend);
  int32_t* heads = (int32_t*)(ws + w.heads);
  int32_t* nheads = (int32_t*)(ws + w.nheads);
  int32_t* deg = (int32_t*)(ws + w.deg);
  const int nb = (int)((N + 255) / 256);
  hipLaunchKernelGGL(rg_keys_kernel<PBC>, dim3(nb), dim3(256), 0, s, pos, N, g, keys, idx, pb);
  size_t cb = w.cub_bytes;
  (void)hipGetLastError();
  E3_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(ws + w.cub, cb, keys, skeys, idx, perm, (int)N, 0, 3 * p->bits, s));
  size_t ncode = (size_t)1 << (3 * p->bits);
  E3_HIP_CHECK(hipMemsetAsync(cbegin, 0, ncode * 4, s));
  E3_HIP_CHECK(hipMemsetAsync(cend, 0, ncode * 4, s));
  E3_HIP_CHECK(hipMemsetAsync(nheads, 0, 4, s));
  hipLaunchKernelGGL(rg_cells_kernel<PBC>, dim3(nb), dim3(256), 0, s, pos, N, skeys, perm, (float4*)sorted_pos4, cbegin,
                     cend, heads, nheads, g, pb);
  const int grid = (int)std::min<int64_t>(N, 256 * 40);
  hipLaunchKernelGGL((rg_scan_kernel<false, PBC>), dim3(grid), dim3(64), 0, s, (const float4*)sorted_pos4, skeys, cbegin,
                     cend, heads, nheads, g, deg, (const int32_t*)nullptr, (int32_t*)nullptr, pb);
  E3_HIP_CHECK(hipMemsetAsync(deg + N, 0, 4, s));
  E3_HIP_CHECK(exclusive_sum(ws + w.cub, w.cub_bytes, deg, rowptr, N + 1, s));
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

template <int PBC>
static int rg_fill(int64_t N, const e3_rg_params* p, const typename RgArg<PBC>::type& pb, const float* sorted_pos4,
                   const int32_t* rowptr, int32_t* src, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p || N < 0 || p->bits < 1 || p->bits > 8) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!sorted_pos4 || !rowptr || !workspace) return E3_ERR_INVALID_ARG;
  RgWs w = rg_ws(N, p->bits);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  RgDev g = rg_dev(p);
  int32_t* deg = (int32_t*)(ws + w.deg);  // reused as the per-row fill cursor between chunks
  const int grid = (int)std::min<int64_t>(N, 256 * 40);
  hipLaunchKernelGGL((rg_scan_kernel<true, PBC>), dim3(grid), dim3(64), 0, s, (const float4*)sorted_pos4,
                     (const uint32_t*)(ws + w.skeys), (const int32_t*)(ws + w.cbegin), (const int32_t*)(ws + w.cend),
                     (const int32_t*)(ws + w.heads), (const int32_t*)(ws + w.nheads), g, deg, rowptr, src, pb);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

template <int PBC>
static int rg_fill_nearest(int64_t N, const e3_rg_params* p, const typename RgArg<PBC>::type& pb, const float* sorted_pos4,
                           const int32_t* rowptr_capped, int k, int32_t* src, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  if (!p || N < 0 || p->bits < 1 || p->bits > 8 || k < 1 || k > 64) return E3_ERR_INVALID_ARG;
  if (N == 0) return E3_OK;
  if (!sorted_pos4 || !rowptr_capped || !src || !workspace) return E3_ERR_INVALID_ARG;
  RgWs w = rg_ws(N, p->bits);
  if ((int64_t)w.total > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  RgDev g = rg_dev(p);
  // deg: the full degrees of the count pass (read only); the unsorted keys are dead after the sort: the per-row cursor
  const int grid = (int)std::min<int64_t>(N, 256 * 40);
  hipLaunchKernelGGL((rg_nearest_kernel<PBC>), dim3(grid), dim3(64), 0, s, (const float4*)sorted_pos4,
                     (const uint32_t*)(ws + w.skeys), (const int32_t*)(ws + w.cbegin), (const int32_t*)(ws + w.cend),
                     (const int32_t*)(ws + w.heads), (const int32_t*)(ws + w.nheads), g, (const int32_t*)(ws + w.deg),
                     (int32_t*)(ws + w.keys), rowptr_capped, src, k, pb);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

static size_t rg_cap_deg_bytes(int64_t N) { return ((size_t)(N + 1) * 4 + 255) / 256 * 256; }

extern "C" {

int64_t e3_rg_cap_workspace_bytes(int64_t N) {
  if (N < 0 || N >= (1ll << 31) - 2) return -1;
  return (int64_t)(rg_cap_deg_bytes(N) + scan_temp_bytes(N + 1) + 256);
}

int e3_rg_cap_rowptr(const int32_t* rowptr_full, int64_t N, int k, int32_t* rowptr_capped, int64_t* stats,
                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (N < 0 || N >= (1ll << 31) - 2 || k < 1 || k > 64 || !rowptr_full || !rowptr_capped || !stats || !workspace)
    return E3_ERR_INVALID_ARG;
  const size_t degb = rg_cap_deg_bytes(N), tmpb = scan_temp_bytes(N + 1) + 256;
  if ((int64_t)(degb + tmpb) > workspace_bytes) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  int32_t* capdeg = (int32_t*)workspace;
  E3_HIP_CHECK(hipMemsetAsync(stats, 0, 16, s));
  const int grid = (int)std::min<int64_t>((N + 1 + 255) / 256, kCapBlocks);
  hipLaunchKernelGGL(rg_cap_kernel, dim3(grid), dim3(256), 0, s, rowptr_full, N, k, capdeg, (unsigned long long*)stats);
  E3_HIP_CHECK(hipGetLastError());
  // the kernel has read all of rowptr_full before the scan writes: rowptr_capped may be the same buffer
  E3_HIP_CHECK(exclusive_sum((char*)workspace + degb, tmpb, capdeg, rowptr_capped, N + 1, s));
  return E3_OK;
}

int e3_rg_fill_nearest(int64_t N, const e3_rg_params* p, const float* sorted_pos4, const int32_t* rowptr_capped, int k,
                       int32_t* src, void* workspace, int64_t workspace_bytes, void* stream) {
  return rg_fill_nearest<kOpen>(N, p, RgPbc{}, sorted_pos4, rowptr_capped, k, src, workspace, workspace_bytes, stream);
}

int e3_rg_fill_nearest_pbc(int64_t N, const e3_rg_params* p, int32_t periodic, const float* sorted_pos4,
                           const int32_t* rowptr_capped, int k, int32_t* src, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  RgPbc pb;
  const int st = rg_pbc(p, periodic, &pb);
  if (st != E3_OK) return st;
  return rg_fill_nearest<kBox>(N, p, pb, sorted_pos4, rowptr_capped, k, src, workspace, workspace_bytes, stream);
}

int e3_rg_fill_nearest_cell(int64_t N, const e3_rg_params* p, const float cell[9], const float origin[3],
                            const float* sorted_pos4, const int32_t* rowptr_capped, int k, int32_t* src, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  RgCell rc;
  const int st = rg_cell(p, cell, origin, &rc);
  if (st != E3_OK) return st;
  return rg_fill_nearest<kCell>(N, p, rc, sorted_pos4, rowptr_capped, k, src, workspace, workspace_bytes, stream);
}

int e3_rg_sort_count(const float* pos, int64_t N, const e3_rg_params* p, int32_t* perm, float* sorted_pos4,
                     int32_t* rowptr, void* workspace, int64_t workspace_bytes, void* stream) {
  return rg_sort_count<kOpen>(pos, N, p, RgPbc{}, perm, sorted_pos4, rowptr, workspace, workspace_bytes, stream);
}

int e3_rg_fill(int64_t N, const e3_rg_params* p, const float* sorted_pos4, const int32_t* rowptr, int32_t* src,
               void* workspace, int64_t workspace_bytes, void* stream) {
  return rg_fill<kOpen>(N, p, RgPbc{}, sorted_pos4, rowptr, src, workspace, workspace_bytes, stream);
}

int e3_rg_sort_count_pbc(const float* pos, int64_t N, const e3_rg_params* p, int32_t periodic, int32_t* perm,
                         float* sorted_pos4, int32_t* rowptr, void* workspace, int64_t workspace_bytes, void* stream) {
  RgPbc pb;
  const int st = rg_pbc(p, periodic, &pb);
  if (st != E3_OK) return st;
  return rg_sort_count<kBox>(pos, N, p, pb, perm, sorted_pos4, rowptr, workspace, workspace_bytes, stream);
}

int e3_rg_fill_pbc(int64_t N, const e3_rg_params* p, int32_t periodic, const float* sorted_pos4, const int32_t* rowptr,
                   int32_t* src, void* workspace, int64_t workspace_bytes, void* stream) {
  RgPbc pb;
  const int st = rg_pbc(p, periodic, &pb);
  if (st != E3_OK) return st;
  return rg_fill<kBox>(N, p, pb, sorted_pos4, rowptr, src, workspace, workspace_bytes, stream);
}

int e3_rg_sort_count_cell(const float* pos, int64_t N, const e3_rg_params* p, const float cell[9], const float origin[3],
                          int32_t* perm, float* sorted_pos4, int32_t* rowptr, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  RgCell rc;
  const int st = rg_cell(p, cell, origin, &rc);
  if (st != E3_OK) return st;
  return rg_sort_count<kCell>(pos, N, p, rc, perm, sorted_pos4, rowptr, workspace, workspace_bytes, stream);
}

int e3_rg_fill_cell(int64_t N, const e3_rg_params* p, const float cell[9], const float origin[3], const float* sorted_pos4,
                    const int32_t* rowptr, int32_t* src, void* workspace, int64_t workspace_bytes, void* stream) {
  RgCell rc;
  const int st = rg_cell(p, cell, origin, &rc);
  if (st != E3_OK) return st;
  return rg_fill<kCell>(N, p, rc, sorted_pos4, rowptr, src, workspace, workspace_bytes, stream);
}

}  // extern "C"
