// Owned sums (e3_msg_forward_owned*): the two small kernels behind the weights-stationary message launch.  Together with it
// they write every row of `out` exactly once (the ownership rule stands above `flush` in e3_msg_ws.hip):
//   msg_boundary_merge_kernel   the first and the last flushed node of every chunk, from their partial sums
//   msg_isolated_rows_kernel    nodes without an incoming edge
#include "e3_msg_plan.h"

#include <algorithm>

namespace e3 {
#include "e3_tp_mfma_core.h"

constexpr int kMergeMaxQ = 5;  // columns per lane: D <= 320 (the weights-stationary kernel has D = 288)

// Boundary merge: the slots part_node[0 .. nslots) = head(0), tail(0), head(1), ... are in edge order; -1 = not filled.
// Consecutive filled slots with the same node are the partial sums of one row (a node that spans k chunks has up to k + 1 of
// them, across empty slots and empty eighths).  A wave per slot i (grid-stride); the wave of a row's FIRST slot sums the parts in slot
// order, stores the row and joins max |row| (finite values) into the max-bits word.
// The wave looks at the ids of slots i - 32 .. i + 31 with ONE load (lane l: slot i - 32 + l) and decides by ballots where
// the row starts and which slots belong to it; the serial walks remain for rows and gaps that leave that window.  The loads
// of the first two parts -- all there is for a node with at most two partial sums -- are issued together.
__global__ __launch_bounds__(256) void msg_boundary_merge_kernel(const float* __restrict__ part,
                                                                 const int* __restrict__ part_node, int64_t nslots, int D,
                                                                 float* __restrict__ out, int64_t ldo, uint32_t* amax) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float m = 0.f;  // running max of the rows this wave stores
  for (int64_t i = wave; i < nslots; i += nwaves) {  // wave-uniform
  const int64_t w0 = i - 32, jl = w0 + lane;
  const int pn = (jl >= 0 && jl < nslots) ? part_node[jl] : -1;
  const int node = __shfl(pn, 32);
  if (node < 0) continue;
  const unsigned long long filled = __ballot(pn >= 0);
  const unsigned long long before = filled & 0xffffffffull;
  bool leader = true;
  if (before) {  // the previous filled slot decides whether this one starts a row
    leader = __shfl(pn, 63 - (int)__builtin_clzll(before)) != node;
  } else {
    for (int64_t j = w0 - 1; j >= 0; --j) {
      const int p = part_node[j];
      if (p < 0) continue;
      leader = p != node;
      break;
    }
  }
  if (!leader) continue;
  const unsigned long long after = filled & ~0x1ffffffffull;                       // lanes 33 .. 63
  const unsigned long long other = __ballot(pn >= 0 && pn != node) & after;
  unsigned long long members = other ? after & ((1ull << __builtin_ctzll(other)) - 1) : after;
  const bool open = !other && w0 + 64 < nslots;   // the row may continue behind the window
  const bool two = members != 0;
  const int64_t j1 = w0 + (two ? (int)__builtin_ctzll(members) : 32);
  if (two) members &= members - 1;
  float sum[kMergeMaxQ], second[kMergeMaxQ];
#pragma unroll
  for (int q = 0; q < kMergeMaxQ; ++q) {
    const int c = 64 * q + lane;
    sum[q] = c < D ? part[i * D + c] : 0.f;
    second[q] = (two && c < D) ? part[j1 * D + c] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < kMergeMaxQ; ++q) {
    const int c = 64 * q + lane;
    if (c < D) {
      float v = two ? sum[q] + second[q] : sum[q];
      for (unsigned long long r = members; r; r &= r - 1) v += part[(w0 + (int)__builtin_ctzll(r)) * D + c];
      if (open) {
        for (int64_t j = w0 + 64; j < nslots; ++j) {
          const int p = part_node[j];
          if (p < 0) continue;
          if (p != node) break;
          v += part[j * D + c];
        }
      }
      out[(int64_t)node * ldo + c] = v;
      m = fmax_finite(m, v);
    }
  }
  }
  // one atomic per wave, and only where it can raise the word: atomics on one address are served one at a time (~10 ns each:
  // one per slot took 1.1 ms at 190 k slots).  The word only grows, so a stale read can cost an atomic but never skip one.
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0 && m > 0.f) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, m);
    if (bits > __atomic_load_n(amax, __ATOMIC_RELAXED)) atomicMax(amax, bits);
  }
}

// Isolated rows: nodes without an incoming edge get zeros.  One pass over the (sorted) dst column: the rows between dst[e - 1]
// and dst[e] are written by the wave that reads the pair; the rows before the first and behind the last dst -- the gaps that
// can be long (padding) -- by the whole grid.  Nothing is written when there are none.  E > 0.
__global__ __launch_bounds__(256) void msg_isolated_rows_kernel(const int32_t* __restrict__ dst, int64_t E, int64_t N, int D,
                                                                float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = dst[0], last = dst[E - 1];
  const int64_t nend = (first + (N - 1 - last)) * D;
  for (int64_t u = gt; u < nend; u += nt) {
    const int64_t r = u / D, c = u - r * D;
    out[(r < first ? r : last + 1 + (r - first)) * ldo + c] = 0.f;
  }
  for (int64_t base = gt - lane; base < E; base += nt) {  // wave-uniform trip count
    const int64_t e = base + lane;
    const bool in = e >= 1 && e < E;
    const int a = in ? dst[e - 1] : 0, b = in ? dst[e] : 0;
    unsigned long long gaps = __ballot(in && b - a > 1);
    while (gaps) {
      const int l = (int)__builtin_ctzll(gaps);
      gaps &= gaps - 1;
      const int64_t ra = __shfl(a, l), rb = __shfl(b, l);
      const int64_t units = (rb - ra - 1) * D;
      for (int64_t u = lane; u < units; u += 64) {
        const int64_t r = u / D, c = u - r * D;
        out[(ra + 1 + r) * ldo + c] = 0.f;
      }
    }
  }
}

int msg_owned_finish(const float* part, const int* part_node, int64_t nslots, const int32_t* dst, int64_t E, int64_t N, int D,
                     float* out, int64_t ldo, uint32_t* amax, hipStream_t s) {
  if (D > 64 * kMergeMaxQ || E <= 0 || nslots <= 0 || (nslots + 3) / 4 > 0x7fffffffLL) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(msg_boundary_merge_kernel, dim3((unsigned)std::min<int64_t>((nslots + 3) / 4, 8192)), dim3(256), 0, s, part, part_node, nslots, D,
                     out, ldo, amax);
  hipLaunchKernelGGL(msg_isolated_rows_kernel, dim3((unsigned)std::min<int64_t>((E + 255) / 256, 4096)), dim3(256), 0, s, dst, E,
                     N, D, out, ldo);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // namespace e3
