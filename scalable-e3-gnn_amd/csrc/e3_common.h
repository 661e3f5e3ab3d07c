// Shared host/device declarations for libe3gnn_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"

namespace e3 {

// ---- error plumbing (e3_lib.hip) ------------------------------------------------------------
void set_hip_error(hipError_t e, const char* what);

#define E3_HIP_CHECK(expr)                                   \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) {                                  \
      ::e3::set_hip_error(_e, #expr);                        \
      return E3_ERR_HIP;                                     \
    }                                                        \
  } while (0)

// The dynamic-LDS limit of a kernel is a per-device attribute of the function, and the library's one place that sets it:
// E3_OK without a HIP call for bytes <= 64 KiB (the default limit); above, the limit of (fn, current device) is raised
// monotonically under one lock -- setting the size of each launch would let two host threads with different plans lower it
// under each other's launches.  E3_ERR_HIP (recorded through set_hip_error) on failure.  e3_lib.hip
int ensure_dyn_lds(const void* fn, size_t bytes);

// ---- element types --------------------------------------------------------------------------
using bf16 = __hip_bfloat16;

template <typename T> struct AccOf { using type = float; };
template <> struct AccOf<double> { using type = double; };

template <typename T> __device__ __forceinline__ typename AccOf<T>::type to_acc(T v) { return v; }
template <> __device__ __forceinline__ float to_acc<bf16>(bf16 v) { return __bfloat162float(v); }

template <typename T, typename A> __device__ __forceinline__ T from_acc(A v) { return static_cast<T>(v); }
template <> __device__ __forceinline__ bf16 from_acc<bf16, float>(float v) { return __float2bfloat16(v); }

// orthorhombic periodic box of the periodic edge kernels (the *_pbc entries): per axis the box length L and 1 / L, both 0 on
// an open axis (the minimum image below is then the identity)
struct PbcBox {
  float L[3], invL[3];
};
// minimum image of one component d = x_src - x_dst: d - L rint(d / L), explicitly rounded (include/e3gnn.h); d for L = 0
__device__ __forceinline__ float min_image(const float d, const float L, const float invL) {
  return __fsub_rn(d, __fmul_rn(L, rintf(__fmul_rn(d, invL))));
}
// a coordinate of a periodic axis wrapped into [lo, hi): w = p - L floor((p - lo) / L), then one correction step
// (include/e3gnn.h above e3_rg_sort_count_pbc; shared by the graph builder and the halo's image selection)
__device__ __forceinline__ float wrap_coord(const float p, const float lo, const float hi, const float L, const float invL) {
  float w = __fsub_rn(p, __fmul_rn(L, floorf(__fmul_rn(__fsub_rn(p, lo), invL))));
  if (w >= hi) w = __fsub_rn(w, L);
  else if (w < lo) w = __fadd_rn(w, L);
  return w;
}
// cell grid of the graph builder (include/e3gnn.h, e3_rg_sort_count), shared with the Morton partition of the sharded path:
// 30-bit Morton interleave of the cell coordinates (x lowest bit) and the cell of one coordinate, explicitly rounded
__host__ __device__ inline uint32_t spread3(uint32_t v) {  // 10 bits -> every third bit
  v &= 0x3ff;
  v = (v | (v << 16)) & 0x030000FF;
  v = (v | (v << 8)) & 0x0300F00F;
  v = (v | (v << 4)) & 0x030C30C3;
  v = (v | (v << 2)) & 0x09249249;
  return v;
}
__host__ __device__ inline uint32_t morton3(int cx, int cy, int cz) {
  return spread3((uint32_t)cx) | (spread3((uint32_t)cy) << 1) | (spread3((uint32_t)cz) << 2);
}
__device__ __forceinline__ int cell_of(float p, float lo, float inv, int n) {
  float t = __fmul_rn(__fsub_rn(p, lo), inv);
  int c = (int)floorf(t);
  return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
}
// general (triclinic) periodic cell of the *_cell entries, periodic on all three lattice directions: h = the lattice vectors
// (row a = a_a, row-major), g = fl32(h^-1) (row-major: the fractional coordinate is s_a = sum_c p_c g[3 c + a])
struct PbcCell {
  float h[9], g[9];
};
// periodicity of a kernel instantiation: open box, orthorhombic box (PbcBox), general cell (PbcCell); kOpen / kBox keep the
// values of the former bool flag.  PbcArg<MODE>: the kernel argument of a mode (the open kernels carry an unread PbcBox)
enum PbcMode : int { kOpen = 0, kBox = 1, kCell = 2 };
template <int MODE> struct PbcArg { using type = PbcBox; };
template <> struct PbcArg<kCell> { using type = PbcCell; };
// fractional component a of a Cartesian vector, explicitly rounded: fl(fl(fl(x g0a) + fl(y g1a)) + fl(z g2a))
__device__ __forceinline__ float cell_frac(const PbcCell& c, const int a, const float x, const float y, const float z) {
  return __fadd_rn(__fadd_rn(__fmul_rn(x, c.g[a]), __fmul_rn(y, c.g[3 + a])), __fmul_rn(z, c.g[6 + a]));
}
// d <- d - (n0 a_0 + n1 a_1 + n2 a_2), per component fl(d_c - fl(fl(fl(n0 h0c) + fl(n1 h1c)) + fl(n2 h2c)))
__device__ __forceinline__ void cell_shift(const PbcCell& c, const float n0, const float n1, const float n2, float& dx,
                                           float& dy, float& dz) {
  dx = __fsub_rn(dx, __fadd_rn(__fadd_rn(__fmul_rn(n0, c.h[0]), __fmul_rn(n1, c.h[3])), __fmul_rn(n2, c.h[6])));
  dy = __fsub_rn(dy, __fadd_rn(__fadd_rn(__fmul_rn(n0, c.h[1]), __fmul_rn(n1, c.h[4])), __fmul_rn(n2, c.h[7])));
  dz = __fsub_rn(dz, __fadd_rn(__fadd_rn(__fmul_rn(n0, c.h[2]), __fmul_rn(n1, c.h[5])), __fmul_rn(n2, c.h[8])));
}
// minimum image of d in a cell (include/e3gnn.h): d - rint(d g) h -- the image with every |ds_a| <= 1/2
__device__ __forceinline__ void min_image(const PbcCell& c, float& dx, float& dy, float& dz) {
  const float n0 = rintf(cell_frac(c, 0, dx, dy, dz)), n1 = rintf(cell_frac(c, 1, dx, dy, dz)),
              n2 = rintf(cell_frac(c, 2, dx, dy, dz));
  cell_shift(c, n0, n1, n2, dx, dy, dz);
}
// general cell (the *_cell entries; include/e3gnn.h): lattice vectors and their inverse, the origin, and the perpendicular
// heights (the grid is the open grid of q_a = s_a h_a in [0, h_a): g.lo = 0, 1 / g.inv = h_a / n_a)
struct RgCell {
  PbcCell c;
  float o[3], hgt[3];
};
// fractional coordinates of p relative to the origin
__device__ __forceinline__ void cell_s(const RgCell& rc, const float3 p, float (&s)[3]) {
  const float x = __fsub_rn(p.x, rc.o[0]), y = __fsub_rn(p.y, rc.o[1]), z = __fsub_rn(p.z, rc.o[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) s[a] = cell_frac(rc.c, a, x, y, z);
}
// p wrapped into the cell: w = p - floor(s(p)) h, then one correction step per lattice direction from s(w)
__device__ __forceinline__ float3 wrap_cell(const RgCell& rc, float3 p) {
  float s[3];
  cell_s(rc, p, s);
  cell_shift(rc.c, floorf(s[0]), floorf(s[1]), floorf(s[2]), p.x, p.y, p.z);
  cell_s(rc, p, s);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float n = s[a] >= 1.0f ? 1.0f : (s[a] < 0.0f ? -1.0f : 0.0f);
    if (n != 0.0f) {
      p.x = __fsub_rn(p.x, __fmul_rn(n, rc.c.h[3 * a + 0]));
      p.y = __fsub_rn(p.y, __fmul_rn(n, rc.c.h[3 * a + 1]));
      p.z = __fsub_rn(p.z, __fmul_rn(n, rc.c.h[3 * a + 2]));
    }
  }
  return p;
}

// edge vector x_src - x_dst of the geometry kernels; kBox / kCell: its minimum image (the rint form, so unwrapped
// coordinates work too)
template <int PBC>
__device__ __forceinline__ void edge_rel(const float4 pj, const float4 pi, const typename PbcArg<PBC>::type& box, float& rx,
                                         float& ry, float& rz) {
  if constexpr (PBC == kCell) {
    rx = __fsub_rn(pj.x, pi.x); ry = __fsub_rn(pj.y, pi.y); rz = __fsub_rn(pj.z, pi.z);
    min_image(box, rx, ry, rz);
  } else if constexpr (PBC == kBox) {
    rx = min_image(__fsub_rn(pj.x, pi.x), box.L[0], box.invL[0]);
    ry = min_image(__fsub_rn(pj.y, pi.y), box.L[1], box.invL[1]);
    rz = min_image(__fsub_rn(pj.z, pi.z), box.L[2], box.invL[2]);
  } else {
    rx = pj.x - pi.x; ry = pj.y - pi.y; rz = pj.z - pi.z;
  }
}

// per-structure strain of the *_strained geometry entries (include/e3gnn.h): eps [S,9] fp32, row-major (eps[3 a + b]);
// sid [N] structure id of each dst row, NULL = every row is structure 0
struct StrainArg {
  const float* eps;
  const int32_t* sid;
  int S;
};
// structure of row i, -1 when its id is outside [0, S) (such a row is neither strained nor reduced).  Called by a whole
// wave on one row: the id is made wave-uniform, so the strain of the row is read with scalar loads into SGPRs
__device__ __forceinline__ int row_structure(const StrainArg& st, const int64_t i) {
  const int s = st.sid ? st.sid[i] : 0;
  return __builtin_amdgcn_readfirstlane((s >= 0 && s < st.S) ? s : -1);
}
// eps of structure s into registers (zero for s = -1: no read)
__device__ __forceinline__ void load_strain(const StrainArg& st, const int s, float e[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) e[k] = s >= 0 ? st.eps[(int64_t)s * 9 + k] : 0.f;
}
// r <- r + eps r
__device__ __forceinline__ void apply_strain(const float e[9], float& rx, float& ry, float& rz) {
  const float x = rx, y = ry, z = rz;
  rx = x + (e[0] * x + e[1] * y + e[2] * z);
  ry = y + (e[3] * x + e[4] * y + e[5] * z);
  rz = z + (e[6] * x + e[7] * y + e[8] * z);
}

// host: box[3] of a *_pbc entry (L per axis, 0 = open): finite, no negative length, and 2 r < L on every periodic axis
inline bool box_valid(const float* box, float r) {
  if (!box) return false;
  for (int a = 0; a < 3; ++a) {
    const float L = box[a];
    if (!(L >= 0.0f) || !(L < 3.0e38f)) return false;
    if (L > 0.0f && !(2.0f * r < L)) return false;
  }
  return true;
}
inline PbcBox make_box(const float* box) {
  PbcBox b = {};
  for (int a = 0; a < 3 && box; ++a) {
    b.L[a] = box[a];
    b.invL[a] = box[a] > 0.0f ? 1.0f / box[a] : 0.0f;
  }
  return b;
}
// host: what a cell[9] (rows = lattice vectors) derives (include/e3gnn.h, e3_cell_derive), in fp64 from the fp32 entries and
// rounded once: ginv = cell^-1 (cofactors over the determinant), heights h_a = 1 / |column a of cell^-1|, volume = |det|.
// false for a NULL, non-finite or singular cell (any derived value zero or non-finite in fp32).  e3_edge_ops.hip
bool cell_derive(const float* cell, float ginv[9], float heights[3], float* volume);
// host: the device cell of a *_cell entry, derived once: false unless the cell is derivable and 2 r < every height (r = 0:
// the geometry entries, which have no cutoff).  `heights` (optional) receives the three perpendicular heights
inline bool make_cell(const float* cell, float r, PbcCell* out, float* heights = nullptr) {
  float hloc[3], v;
  float* h = heights ? heights : hloc;
  if (!cell_derive(cell, out->g, h, &v) || !(r >= 0.0f)) return false;
  for (int a = 0; a < 3; ++a)
    if (!(2.0f * r < h[a])) return false;
  for (int k = 0; k < 9; ++k) out->h[k] = cell[k];
  return true;
}

// host: grid of the one-wave-per-CSR-row stage kernels (256 threads = 4 rows per workgroup, grid-stride above 4096 groups)
inline int wave_grid(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 256 * 16)); }

// block layout of the gate kernels (e3_gate_blocks and its two backwards), passed by value: block i = mul[i] channels of
// degree l[i]; the unused tail has mul = 1 << 30, which ends the kernels' search for the block of a column
struct GateBlocks {
  int nblocks;
  int l[8], mul[8];
};
// host: the descriptor of (ns, nblocks, ls, muls) with the gate count and the output width W = ns + sum mul (2 l + 1);
// E3_ERR_INVALID_ARG for ns < 0, nblocks outside [0, 8], a missing array, l outside [0, 2] or a negative mul
inline int make_gate_blocks(int ns, int nblocks, const int32_t* ls, const int32_t* muls, GateBlocks* gb, int* ngates,
                            int* W) {
  if (ns < 0 || nblocks < 0 || nblocks > 8 || (nblocks > 0 && (!ls || !muls))) return E3_ERR_INVALID_ARG;
  gb->nblocks = nblocks;
  int gates = 0, wide = 0;
  for (int i = 0; i < 8; ++i) { gb->l[i] = 0; gb->mul[i] = 1 << 30; }
  for (int i = 0; i < nblocks; ++i) {
    if (ls[i] < 0 || ls[i] > 2 || muls[i] < 0) return E3_ERR_INVALID_ARG;
    gb->l[i] = ls[i]; gb->mul[i] = muls[i];
    gates += muls[i];
    wide += muls[i] * (2 * ls[i] + 1);
  }
  *ngates = gates;
  *W = ns + wide;
  return E3_OK;
}

// e3_scan.hip: the library's one exclusive prefix sum over int32 (the only instantiation of hipcub's DeviceScan), shared by
// the graph builder, the edge split and the two halo selections.  Temporary storage for n elements (hipcub's own figure, not
// rounded), and out[i] = in[0] + ... + in[i - 1] for i < n on stream s with at least that much at `temp`
size_t scan_temp_bytes(int64_t n);
hipError_t exclusive_sum(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t s);
}  // namespace e3
