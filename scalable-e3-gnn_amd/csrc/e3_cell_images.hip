// Small periodic cells (cell_images.CellImages; spec in include/e3gnn.h, "Image rows"): the cloud of a cell below twice the
// cutoff is extended by explicit lattice images and the graph over it stays OPEN.  Three pieces, integer / HBM work, no MFMA:
//   selection : one thread per particle.  The slab rule is separable, so a particle's kept shifts are a product of three
//               per-axis sets (a 15-bit mask each, shifts -7 .. 7); the count is the product of the three popcounts minus the
//               zero shift, ONE exclusive scan (e3_scan.hip) over the N + 1 counts gives every particle its output offset
//               and the total, and the fill pass recomputes the masks and walks them in lexicographic order -- the output
//               is ordered by (owner, shift) by construction, no atomics.  The batched form (many cells per call) is the same
//               pair with the cell read per particle from a table of records; the single-cell kernels are untouched.
//   expand   : out[i] = in[source[i]], one wave per row, 16-byte column groups where every pointer and pitch allows them
//               (the layout of e3_halo_grad.hip); a row copy moves bytes, so one kernel per element SIZE serves fp32, bf16
//               and fp64.  The translated form (positions, D = 3, fp32) is one thread per row.
//   reduce    : the transpose, a row sum over a CSR in the list's order by one wave per row: bit-equal from run to run.
// Compiled without contraction (Makefile): the selection and the translation are compared bit for bit with a restatement
// that rounds every fp32 operation on its own.
#include "e3_rows.h"

#include <cmath>

namespace e3 {

constexpr int kImgThreads = 256;
constexpr int kImgBias = E3_CELL_IMAGE_MAX_SHELLS;   // bit (n + kImgBias) of an axis mask = shift n

struct ImgDev {
  RgCell rc;
  int m[3];
  float rho;
};

// the kept shifts of one axis: n in [-m, m] with fl(fl(s + n) h) >= -rho and fl(fl(fl(s + n) - 1) h) <= rho
__device__ __forceinline__ uint32_t axis_mask(const float s, const float h, const int m, const float rho) {
  uint32_t k = 0;
  for (int n = -m; n <= m; ++n) {
    const float t = __fadd_rn(s, (float)n);
    const bool keep = __fmul_rn(t, h) >= -rho && __fmul_rn(__fsub_rn(t, 1.0f), h) <= rho;
    k |= (keep ? 1u : 0u) << (n + kImgBias);
  }
  return k;
}

__device__ __forceinline__ void image_masks(const ImgDev& d, const float3 w, uint32_t (&k)[3]) {
  float s[3];
  cell_s(d.rc, w, s);
#pragma unroll
  for (int a = 0; a < 3; ++a) k[a] = axis_mask(s[a], d.rc.hgt[a], d.m[a], d.rho);
}

// wrapped positions out; cnt[i] = the images of particle i
__global__ __launch_bounds__(kImgThreads) void images_count_kernel(const float* __restrict__ pos, int64_t n, const ImgDev d,
                                                                   float* __restrict__ pos_w, int32_t* __restrict__ cnt) {
  const int64_t i = blockIdx.x * (int64_t)kImgThreads + threadIdx.x;
  if (i >= n) return;
  const float3 w = wrap_cell(d.rc, make_float3(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2]));
  pos_w[3 * i + 0] = w.x; pos_w[3 * i + 1] = w.y; pos_w[3 * i + 2] = w.z;
  uint32_t k[3];
  image_masks(d, w, k);
  const int zero = (k[0] >> kImgBias) & (k[1] >> kImgBias) & (k[2] >> kImgBias) & 1;
  cnt[i] = __popc(k[0]) * __popc(k[1]) * __popc(k[2]) - zero;
}

__global__ __launch_bounds__(kImgThreads) void images_fill_kernel(const float* __restrict__ pos_w, int64_t n, const ImgDev d,
                                                                  const int32_t* __restrict__ off, int64_t total,
                                                                  int32_t* __restrict__ owner, int32_t* __restrict__ shift,
                                                                  float* __restrict__ image_pos) {
  const int64_t i = blockIdx.x * (int64_t)kImgThreads + threadIdx.x;
  if (i >= n) return;
  const float3 w = make_float3(pos_w[3 * i + 0], pos_w[3 * i + 1], pos_w[3 * i + 2]);
  uint32_t k[3];
  image_masks(d, w, k);
  int64_t o = off[i];
  const int64_t end = off[i + 1] < total ? off[i + 1] : total;   // a caller that changed the inputs between the calls writes
  for (int n0 = -d.m[0]; n0 <= d.m[0]; ++n0) {                  // nothing past its own rows and nothing past the arrays
    if (!((k[0] >> (n0 + kImgBias)) & 1)) continue;
    for (int n1 = -d.m[1]; n1 <= d.m[1]; ++n1) {
      if (!((k[1] >> (n1 + kImgBias)) & 1)) continue;
      for (int n2 = -d.m[2]; n2 <= d.m[2]; ++n2) {
        if (!((k[2] >> (n2 + kImgBias)) & 1) || (n0 == 0 && n1 == 0 && n2 == 0)) continue;
        if (o < 0 || o >= end) return;
        float x = w.x, y = w.y, z = w.z;
        cell_shift(d.rc.c, (float)-n0, (float)-n1, (float)-n2, x, y, z);   // w + n cell, rounded as the shift rounds
        owner[o] = (int32_t)i;
        shift[3 * o + 0] = n0; shift[3 * o + 1] = n1; shift[3 * o + 2] = n2;
        image_pos[3 * o + 0] = x; image_pos[3 * o + 1] = y; image_pos[3 * o + 2] = z;
        ++o;
      }
    }
  }
}

// ---- batches of cells: the same selection with the cell looked up per particle -----------------------------------------
// One record per structure in a device table the caller uploads (e3_cell_images_plan_batch fills the host copy): the ImgDev of
// the single-cell kernels, 112 bytes = seven 16-byte groups.  Still one thread per particle: the work of a particle is its own
// wrap and three axis masks, nothing is shared between the particles of a structure but the record, and neighbouring
// particles usually share a structure, so a wave's seven loads hit the same one or two lines.
struct alignas(16) ImgRec {
  ImgDev d;
};
static_assert(sizeof(ImgDev) == 112 && sizeof(ImgRec) == E3_CELL_IMAGE_RECORD_BYTES && sizeof(ImgRec) % 16 == 0,
              "the table record is the single-cell kernel argument, in whole 16-byte groups");

// the record of structure s (s inside [0, B): the caller checks), seven 16-byte loads; false for a record the masks cannot
// hold (more than kImgBias shells: the host entries refuse it, a table changed behind them selects nothing)
__device__ __forceinline__ bool load_record(const ImgRec* __restrict__ table, const int s, ImgDev& d) {
  constexpr int kGroups = sizeof(ImgRec) / 16;
  uint4 q[kGroups];
  const uint4* p = reinterpret_cast<const uint4*>(table + s);
#pragma unroll
  for (int k = 0; k < kGroups; ++k) q[k] = p[k];
  __builtin_memcpy(&d, q, sizeof(ImgDev));
  return d.m[0] >= 1 && d.m[1] >= 1 && d.m[2] >= 1 && d.m[0] <= kImgBias && d.m[1] <= kImgBias && d.m[2] <= kImgBias;
}

// a structure id outside [0, B): count 0, the position kept as it is
__global__ __launch_bounds__(kImgThreads) void images_count_batch_kernel(const float* __restrict__ pos,
                                                                         const int32_t* __restrict__ structure, int64_t n,
                                                                         const ImgRec* __restrict__ table, int B,
                                                                         float* __restrict__ pos_w, int32_t* __restrict__ cnt) {
  const int64_t i = blockIdx.x * (int64_t)kImgThreads + threadIdx.x;
  if (i >= n) return;
  float3 w = make_float3(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2]);
  const int s = structure[i];
  ImgDev d;
  int c = 0;
  if (s >= 0 && s < B && load_record(table, s, d)) {
    w = wrap_cell(d.rc, w);
    uint32_t k[3];
    image_masks(d, w, k);
    const int zero = (k[0] >> kImgBias) & (k[1] >> kImgBias) & (k[2] >> kImgBias) & 1;
    c = __popc(k[0]) * __popc(k[1]) * __popc(k[2]) - zero;
  }
  pos_w[3 * i + 0] = w.x; pos_w[3 * i + 1] = w.y; pos_w[3 * i + 2] = w.z;
  cnt[i] = c;
}

__global__ __launch_bounds__(kImgThreads) void images_fill_batch_kernel(const float* __restrict__ pos_w,
                                                                        const int32_t* __restrict__ structure, int64_t n,
                                                                        const ImgRec* __restrict__ table, int B,
                                                                        const int32_t* __restrict__ off, int64_t total,
                                                                        int32_t* __restrict__ owner, int32_t* __restrict__ shift,
                                                                        float* __restrict__ image_pos) {
  const int64_t i = blockIdx.x * (int64_t)kImgThreads + threadIdx.x;
  if (i >= n) return;
  const int s = structure[i];
  ImgDev d;
  if (s < 0 || s >= B || !load_record(table, s, d)) return;
  const float3 w = make_float3(pos_w[3 * i + 0], pos_w[3 * i + 1], pos_w[3 * i + 2]);
  uint32_t k[3];
  image_masks(d, w, k);
  int64_t o = off[i];
  const int64_t end = off[i + 1] < total ? off[i + 1] : total;   // as the single-cell fill: nothing past the particle's own
  for (int n0 = -d.m[0]; n0 <= d.m[0]; ++n0) {                  // rows and nothing past the arrays
    if (!((k[0] >> (n0 + kImgBias)) & 1)) continue;
    for (int n1 = -d.m[1]; n1 <= d.m[1]; ++n1) {
      if (!((k[1] >> (n1 + kImgBias)) & 1)) continue;
      for (int n2 = -d.m[2]; n2 <= d.m[2]; ++n2) {
        if (!((k[2] >> (n2 + kImgBias)) & 1) || (n0 == 0 && n1 == 0 && n2 == 0)) continue;
        if (o < 0 || o >= end) return;
        float x = w.x, y = w.y, z = w.z;
        cell_shift(d.rc.c, (float)-n0, (float)-n1, (float)-n2, x, y, z);
        owner[o] = (int32_t)i;
        shift[3 * o + 0] = n0; shift[3 * o + 1] = n1; shift[3 * o + 2] = n2;
        image_pos[3 * o + 0] = x; image_pos[3 * o + 1] = y; image_pos[3 * o + 2] = z;
        ++o;
      }
    }
  }
}

// host: shells and margin (include/e3gnn.h).  E3_ERR_INVALID_ARG for a cell that does not derive, a non-finite origin or an
// r that is not finite and positive.  The shells are reported as they are (capped at 2^20): shells_ok is the limit
static int image_plan(const float* cell, const float* origin, float r, ImgDev* d) {
  float vol;
  if (!origin || !cell_derive(cell, d->rc.c.g, d->rc.hgt, &vol) || !(r > 0.0f) || !(r < 3.0e38f)) return E3_ERR_INVALID_ARG;
  double size = (double)r;
  for (int k = 0; k < 9; ++k) {
    d->rc.c.h[k] = cell[k];
    size += fabs((double)cell[k]);
  }
  for (int a = 0; a < 3; ++a) {
    if (!(fabsf(origin[a]) < 3.0e38f)) return E3_ERR_INVALID_ARG;
    d->rc.o[a] = origin[a];
    size += fabs((double)origin[a]);
  }
  const double rho = (double)r + size * (1.0 / 262144.0);   // 2^-18 = 64 ulp of everything a coordinate can reach
  d->rho = (float)rho;
  if ((double)d->rho < rho) d->rho = nextafterf(d->rho, INFINITY);
  if (!(d->rho < 3.0e38f)) return E3_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a) {
    const double m = ceil((double)d->rho / (double)d->rc.hgt[a]);
    d->m[a] = m < 1.0 ? 1 : (m < 1048576.0 ? (int)m : 1048576);
  }
  return E3_OK;
}

// the kernels' axis masks hold the shifts -7 .. 7
static bool shells_ok(const ImgDev& d) {
  return d.m[0] <= E3_CELL_IMAGE_MAX_SHELLS && d.m[1] <= E3_CELL_IMAGE_MAX_SHELLS && d.m[2] <= E3_CELL_IMAGE_MAX_SHELLS;
}

// every count, every offset and N + G fit an int32 whatever the positions are
static bool image_sizes_ok(int64_t n, const ImgDev& d) {
  const int64_t per = (int64_t)(2 * d.m[0] + 1) * (2 * d.m[1] + 1) * (2 * d.m[2] + 1);
  return n >= 0 && n * per < 0x7fffffffLL;
}

// a batch: the host copy of the table and the particles per structure.  Every structure inside the shell limit, the counts
// non-negative with sum N, and sum_b counts[b] (2 m_0 + 1)(2 m_1 + 1)(2 m_2 + 1) < 2^31 - 1 with each structure's own shells
static bool batch_sizes_ok(const ImgRec* host, const int64_t* counts, int64_t B, int64_t n) {
  if (B < 0 || B >= 0x7fffffffLL || n < 0 || (B > 0 && (!host || !counts))) return false;
  int64_t atoms = 0, rows = 0;
  for (int64_t b = 0; b < B; ++b) {
    const ImgDev& d = host[b].d;
    if (!shells_ok(d) || d.m[0] < 1 || d.m[1] < 1 || d.m[2] < 1 || counts[b] < 0 || counts[b] >= 0x7fffffffLL) return false;
    atoms += counts[b];
    rows += counts[b] * ((int64_t)(2 * d.m[0] + 1) * (2 * d.m[1] + 1) * (2 * d.m[2] + 1));
    if (atoms >= 0x7fffffffLL || rows >= 0x7fffffffLL) return false;
  }
  return atoms == n;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline int img_blocks(int64_t n) { return (int)((n + kImgThreads - 1) / kImgThreads); }

// workspace: cnt [n + 1] | scan temp
static inline size_t img_cnt_bytes(int64_t n) { return ((size_t)(n + 1) * 4 + 255) / 256 * 256; }

// ---- rows ------------------------------------------------------------------------------------------------------------
template <int ES> struct Word;
template <> struct Word<2> { using type = uint16_t; };
template <> struct Word<4> { using type = uint32_t; };
template <> struct Word<8> { using type = uint64_t; };

// out[i] = in[source[i]] (a source outside [0, M) writes a zero row).  IMAGES_ONLY: rows with source[i] == i are left alone
// (the in-place form, out == in: an image row is never a source, so no row is read after it was written).
// DV = the 16-byte groups of a row (0: every column goes through the element loop)
template <int ES, bool IMAGES_ONLY>
__global__ __launch_bounds__(256) void rows_expand_kernel(const void* in_, int64_t ld_i,
                                                          const int32_t* __restrict__ source, int64_t M, int DV, int D,
                                                          void* out_, int64_t ld_o) {
  using T = typename Word<ES>::type;
  constexpr int VW = 16 / ES;
  const T* in = static_cast<const T*>(in_);
  T* out = static_cast<T*>(out_);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < M; i += nw) {
    const int64_t s = source[i];
    if (IMAGES_ONLY && s == i) continue;
    const T* src = (s >= 0 && s < M) ? in + s * ld_i : nullptr;
    T* dst = out + i * ld_o;
    for (int c = lane; c < DV; c += 64)
      reinterpret_cast<uint4*>(dst)[c] = src ? reinterpret_cast<const uint4*>(src)[c] : make_uint4(0u, 0u, 0u, 0u);
    for (int c = DV * VW + lane; c < D; c += 64) dst[c] = src ? src[c] : T(0);
  }
}

// positions: out[i] = in[source[i]] + shift[i] cell, per component as cell_shift rounds; one thread per row
template <bool IMAGES_ONLY>
__global__ __launch_bounds__(256) void rows_translate_kernel(const float* in, int64_t ld_i,
                                                             const int32_t* __restrict__ source,
                                                             const int32_t* __restrict__ shift, const PbcCell c, int64_t M,
                                                             float* out, int64_t ld_o) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= M) return;
  const int64_t s = source[i];
  if (IMAGES_ONLY && s == i) return;
  float x = 0.f, y = 0.f, z = 0.f;
  if (s >= 0 && s < M) {
    x = in[s * ld_i + 0]; y = in[s * ld_i + 1]; z = in[s * ld_i + 2];
    cell_shift(c, (float)-shift[3 * i + 0], (float)-shift[3 * i + 1], (float)-shift[3 * i + 2], x, y, z);
  }
  out[i * ld_o + 0] = x; out[i * ld_o + 1] = y; out[i * ld_o + 2] = z;
}


// out[i] = source[i] == i ? g[i] + sum_{q in [ptr[i], ptr[i+1])} g[rows[q]] : 0, added in q order in T.  The list bounds are
// clamped to [0, n_rows] and a row id outside [0, M) adds nothing: nothing is read out of bounds.
template <typename T>
__global__ __launch_bounds__(256) void rows_reduce_kernel(const T* __restrict__ g, int64_t ld_g,
                                                          const int32_t* __restrict__ source, const int32_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ rows, int64_t n_rows, int64_t M, int DV,
                                                          int D, T* __restrict__ out, int64_t ld_o) {
  using V = typename Vec16<T>::type;
  constexpr int VW = sizeof(V) / sizeof(T);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t i = blockIdx.x * (int64_t)4 + wid; i < M; i += nw) {
    const bool owned = source[i] == i;
    int64_t b = 0, e = 0;
    if (owned && n_rows > 0) {
      b = ptr[i] < 0 ? 0 : ptr[i];
      e = ptr[i + 1] > n_rows ? n_rows : ptr[i + 1];
    }
    const T* grow = g + i * ld_g;
    T* dst = out + i * ld_o;
    for (int c = lane; c < DV; c += 64) {
      V acc;
      vclear(acc);
      if (owned) acc = reinterpret_cast<const V*>(grow)[c];
#pragma unroll 4
      for (int64_t q = b; q < e; ++q) {
        const int64_t j = rows[q];
        if (j >= 0 && j < M) vadd(acc, reinterpret_cast<const V*>(g + j * ld_g)[c]);
      }
      reinterpret_cast<V*>(dst)[c] = acc;
    }
    for (int c = DV * VW + lane; c < D; c += 64) {
      T acc = owned ? grow[c] : T(0);
#pragma unroll 4
      for (int64_t q = b; q < e; ++q) {
        const int64_t j = rows[q];
        if (j >= 0 && j < M) acc += g[j * ld_g + c];
      }
      dst[c] = acc;
    }
  }
}

template <int ES>
static int expand_launch(const void* in, int64_t ld_in, const int32_t* source, int64_t M, int D, void* out, int64_t ld_out,
                         hipStream_t s) {
  const int DV = groups16(D, ES, {in, out}, {ld_in, ld_out});
  if (in == out)
    hipLaunchKernelGGL((rows_expand_kernel<ES, true>), dim3(wave_grid(M)), dim3(256), 0, s, in, ld_in, source, M, DV, D, out,
                       ld_out);
  else
    hipLaunchKernelGGL((rows_expand_kernel<ES, false>), dim3(wave_grid(M)), dim3(256), 0, s, in, ld_in, source, M, DV, D, out,
                       ld_out);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

template <typename T>
static int reduce_launch(const void* g, int64_t ld_g, const int32_t* source, const int32_t* ptr, const int32_t* rows,
                         int64_t n_rows, int64_t M, int D, void* out, int64_t ld_out, hipStream_t s) {
  const int DV = groups16(D, sizeof(T), {g, out}, {ld_g, ld_out});
  hipLaunchKernelGGL(rows_reduce_kernel<T>, dim3(wave_grid(M)), dim3(256), 0, s, (const T*)g, ld_g, source, ptr, rows, n_rows,
                     M, DV, D, (T*)out, ld_out);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_cell_images_plan(const float cell[9], const float origin[3], float r, int32_t shells[3], float* rho) {
  ImgDev d;
  if (!shells || !rho) return E3_ERR_INVALID_ARG;
  const int st = image_plan(cell, origin, r, &d);
  if (st != E3_OK) return st;
  for (int a = 0; a < 3; ++a) shells[a] = d.m[a];
  *rho = d.rho;
  return E3_OK;
}

int64_t e3_cell_images_workspace_bytes(int64_t N) {
  if (N < 0 || N >= 0x7fffffffLL) return -1;
  return (int64_t)(img_cnt_bytes(N) + (scan_temp_bytes(N + 1) + 255) / 256 * 256);
}

int e3_cell_images_count(const float* pos, int64_t N, const float cell[9], const float origin[3], float r, float* pos_wrapped,
                         int32_t* offsets, void* workspace, int64_t workspace_bytes, void* stream) {
  ImgDev d;
  const int st = image_plan(cell, origin, r, &d);
  if (st != E3_OK) return st;
  if (!shells_ok(d) || !image_sizes_ok(N, d) || !offsets || !workspace || (N > 0 && (!pos || !pos_wrapped)))
    return E3_ERR_INVALID_ARG;
  if (workspace_bytes < e3_cell_images_workspace_bytes(N)) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    E3_HIP_CHECK(hipMemsetAsync(offsets, 0, 4, s));
    return E3_OK;
  }
  int32_t* cnt = static_cast<int32_t*>(workspace);
  E3_HIP_CHECK(hipMemsetAsync(cnt + N, 0, 4, s));
  hipLaunchKernelGGL(images_count_kernel, dim3(img_blocks(N)), dim3(kImgThreads), 0, s, pos, N, d, pos_wrapped, cnt);
  E3_HIP_CHECK(hipGetLastError());
  E3_HIP_CHECK(exclusive_sum(static_cast<char*>(workspace) + img_cnt_bytes(N), scan_temp_bytes(N + 1), cnt, offsets, N + 1, s));
  return E3_OK;
}

int e3_cell_images_fill(const float* pos_wrapped, int64_t N, const float cell[9], const float origin[3], float r,
                        const int32_t* offsets, int64_t G, int32_t* owner, int32_t* shift, float* image_pos, void* stream) {
  ImgDev d;
  const int st = image_plan(cell, origin, r, &d);
  if (st != E3_OK) return st;
  if (!shells_ok(d) || !image_sizes_ok(N, d) || G < 0 || N + G >= 0x7fffffffLL) return E3_ERR_INVALID_ARG;
  if (N == 0 || G == 0) return E3_OK;
  if (!pos_wrapped || !offsets || !owner || !shift || !image_pos) return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(images_fill_kernel, dim3(img_blocks(N)), dim3(kImgThreads), 0, (hipStream_t)stream, pos_wrapped, N, d,
                     offsets, G, owner, shift, image_pos);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int64_t e3_cell_images_record_bytes(void) { return (int64_t)sizeof(ImgRec); }

int e3_cell_images_plan_batch(const float* cells, const float* origins, int64_t B, float r, int32_t* shells, float* rho,
                              void* table) {
  if (B < 0 || B >= 0x7fffffffLL || !cells || !origins || !shells || !rho || !table || !aligned16(table))
    return E3_ERR_INVALID_ARG;
  ImgRec* rec = static_cast<ImgRec*>(table);
  for (int64_t b = 0; b < B; ++b) {
    ImgDev d;
    const int st = image_plan(cells + 9 * b, origins + 3 * b, r, &d);
    if (st != E3_OK) return st;
    for (int a = 0; a < 3; ++a) shells[3 * b + a] = d.m[a];
    rho[b] = d.rho;
    rec[b].d = d;
  }
  return E3_OK;
}

int e3_cell_images_count_batch(const float* pos, const int32_t* structure, int64_t N, const void* table,
                               const void* table_host, const int64_t* counts, int64_t B, float* pos_wrapped, int32_t* offsets,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!batch_sizes_ok(static_cast<const ImgRec*>(table_host), counts, B, N) || !offsets || !workspace ||
      (N > 0 && (!pos || !structure || !pos_wrapped || !table || !aligned16(table))))
    return E3_ERR_INVALID_ARG;
  if (workspace_bytes < e3_cell_images_workspace_bytes(N)) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    E3_HIP_CHECK(hipMemsetAsync(offsets, 0, 4, s));
    return E3_OK;
  }
  int32_t* cnt = static_cast<int32_t*>(workspace);
  E3_HIP_CHECK(hipMemsetAsync(cnt + N, 0, 4, s));
  hipLaunchKernelGGL(images_count_batch_kernel, dim3(img_blocks(N)), dim3(kImgThreads), 0, s, pos, structure, N,
                     static_cast<const ImgRec*>(table), (int)B, pos_wrapped, cnt);
  E3_HIP_CHECK(hipGetLastError());
  E3_HIP_CHECK(exclusive_sum(static_cast<char*>(workspace) + img_cnt_bytes(N), scan_temp_bytes(N + 1), cnt, offsets, N + 1, s));
  return E3_OK;
}

int e3_cell_images_fill_batch(const float* pos_wrapped, const int32_t* structure, int64_t N, const void* table,
                              const void* table_host, const int64_t* counts, int64_t B, const int32_t* offsets, int64_t G,
                              int32_t* owner, int32_t* shift, float* image_pos, void* stream) {
  if (!batch_sizes_ok(static_cast<const ImgRec*>(table_host), counts, B, N) || G < 0 || N + G >= 0x7fffffffLL)
    return E3_ERR_INVALID_ARG;
  if (N == 0 || G == 0) return E3_OK;
  if (!pos_wrapped || !structure || !table || !aligned16(table) || !offsets || !owner || !shift || !image_pos)
    return E3_ERR_INVALID_ARG;
  hipLaunchKernelGGL(images_fill_batch_kernel, dim3(img_blocks(N)), dim3(kImgThreads), 0, (hipStream_t)stream, pos_wrapped,
                     structure, N, static_cast<const ImgRec*>(table), (int)B, offsets, G, owner, shift, image_pos);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

int e3_image_rows_expand(const void* in, int64_t ld_in, const int32_t* source, const int32_t* shift, const float cell[9],
                         int64_t M, int D, int dtype, void* out, int64_t ld_out, void* stream) {
  if (M < 0 || M >= 0x7fffffffLL || D < 1 || ld_in < D || ld_out < D ||
      (dtype != E3_F32 && dtype != E3_F64 && dtype != E3_BF16))
    return E3_ERR_INVALID_ARG;
  if ((shift != nullptr) != (cell != nullptr) || (shift && (D != 3 || dtype != E3_F32))) return E3_ERR_INVALID_ARG;
  if (in == out && ld_in != ld_out) return E3_ERR_INVALID_ARG;
  PbcCell c;
  if (cell && !make_cell(cell, 0.0f, &c)) return E3_ERR_INVALID_ARG;
  if (M == 0) return E3_OK;
  if (!in || !source || !out) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (shift) {
    const dim3 grid((unsigned)((M + 255) / 256));
    if (in == out)
      hipLaunchKernelGGL(rows_translate_kernel<true>, grid, dim3(256), 0, s, (const float*)in, ld_in, source, shift, c, M,
                         (float*)out, ld_out);
    else
      hipLaunchKernelGGL(rows_translate_kernel<false>, grid, dim3(256), 0, s, (const float*)in, ld_in, source, shift, c, M,
                         (float*)out, ld_out);
    E3_HIP_CHECK(hipGetLastError());
    return E3_OK;
  }
  return dtype == E3_BF16  ? expand_launch<2>(in, ld_in, source, M, D, out, ld_out, s)
         : dtype == E3_F32 ? expand_launch<4>(in, ld_in, source, M, D, out, ld_out, s)
                           : expand_launch<8>(in, ld_in, source, M, D, out, ld_out, s);
}

int e3_image_rows_reduce(const void* g, int64_t ld_g, const int32_t* source, const int32_t* ptr, const int32_t* rows,
                         int64_t n_rows, int64_t M, int D, int dtype, void* out, int64_t ld_out, void* stream) {
  if (M < 0 || M >= 0x7fffffffLL || n_rows < 0 || D < 1 || ld_g < D || ld_out < D || (dtype != E3_F32 && dtype != E3_F64))
    return E3_ERR_INVALID_ARG;
  if (M == 0) return E3_OK;
  if (!g || !source || !out || g == out || (n_rows > 0 && (!ptr || !rows))) return E3_ERR_INVALID_ARG;
  return dtype == E3_F32
             ? reduce_launch<float>(g, ld_g, source, ptr, rows, n_rows, M, D, out, ld_out, (hipStream_t)stream)
             : reduce_launch<double>(g, ld_g, source, ptr, rows, n_rows, M, D, out, ld_out, (hipStream_t)stream);
}

}  // extern "C"
