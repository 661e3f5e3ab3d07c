// General SH tensor product for l <= 2 (builder-defined; contract in include/e3gnn.h).  This file: the host plan and its
// queries, the weight pack, the generic FMA forward kernel (fp32 / fp64; it contracts the channel index with W first,
// T[m1] = sum_k W[k,w] x[k,m1], and applies the coupling tensor and Y afterwards) and the e3_tp_forward* entries, which
// hand everything else to the MFMA path (e3_tp_mfma.hip).  Backward: e3_tp_bwd.hip, e3_tp_wgrad.hip.
#include "e3_tp_cg.h"

#include <array>
#include <cstdlib>

namespace e3 {

template <typename T, int R>
__global__ __launch_bounds__(256) void tp_fwd_generic_kernel(const T* __restrict__ in1, int64_t ld1,
                                                             const T* __restrict__ in2, int64_t ld2,
                                                             const typename AccOf<T>::type* __restrict__ packed,
                                                             T* __restrict__ out, int64_t ldo, int64_t B, TpDev p) {
  using A = typename AccOf<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  A* xs = reinterpret_cast<A*>(smem_raw);
  A* ys = xs + (size_t)R * p.D1;
  const int tid = threadIdx.x;
  int Mtot = 0;
  for (int c = 0; c < 6; ++c) Mtot += p.M[c];
  const A* normcol = packed + p.normcol_off;
  const int64_t ntiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    tp_stage_rows<T, A>(in1, ld1, in2, ld2, nullptr, 0, nullptr, row0, R, B, p, xs, ys, nullptr);
    __syncthreads();
    for (int i = tid; i < R * Mtot; i += 256) {
      int r = i / Mtot, w = i - r * Mtot;
      int64_t row = row0 + r;
      if (row >= B) continue;
      int c3 = 0;
      while (w >= p.M[c3]) { w -= p.M[c3]; ++c3; }
      const int l3 = c3 >> 1, M = p.M[c3];
      const A* x = xs + r * p.D1;
      const A* y = ys + r * p.Dy;
      A o[5] = {0, 0, 0, 0, 0};
      for (int pi = 0; pi < p.npath[c3]; ++pi) {
        const TpPath P = p.paths[p.poff[c3] + pi];
        const A* xc = x + p.cbase[P.c1];
        const A* W = packed + p.woff[c3] + (int64_t)P.wrow * M + w;
        const A* yl = y + P.l2 * P.l2;  // offsets 0, 1, 4
        const int n = p.n[P.c1];
        E3_TP_PATH_SWITCH(P.l1, P.l2, l3, G::fwd(xc, n, W, M, yl, o))
      }
      const int oc = p.ocol[p.ocol_off[c3] + w];
      T* dst = out + row * ldo + oc;
      for (int m = 0; m < 2 * l3 + 1; ++m) dst[m] = from_acc<T, A>(o[m] * normcol[oc + m]);
    }
    __syncthreads();
  }
}

// packed generic section: the class matrices (missing = zeros) and the norms scattered to out column order (missing = ones)
template <typename T>
__global__ void tp_pack_kernel(TpPtr6 w, TpPtr6 nr, typename AccOf<T>::type* packed, TpDev p) {
  using A = typename AccOf<T>::type;
  int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int c = 0; c < 6; ++c) {
    const T* wc = static_cast<const T*>(w.p[c]);
    const T* nc = static_cast<const T*>(nr.p[c]);
    int64_t nw = (int64_t)p.K[c] * p.M[c];
    for (int64_t i = tid; i < nw; i += stride) packed[p.woff[c] + i] = wc ? to_acc(wc[i]) : A(0);
    int width = 2 * (c >> 1) + 1;
    for (int64_t i = tid; i < (int64_t)p.M[c] * width; i += stride) {
      int m = (int)(i / width), comp = (int)(i - (int64_t)m * width);
      packed[p.normcol_off + p.ocol[p.ocol_off[c] + m] + comp] = nc ? to_acc(nc[i]) : A(1);
    }
  }
}

int tp_ensure_device(const e3_tp_plan* cplan) {
  auto* P = const_cast<e3_tp_plan*>(cplan);
  std::lock_guard<std::mutex> lock(P->mu);
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return E3_ERR_NO_DEVICE;
  if (P->d_tables) return cur == P->device ? E3_OK : E3_ERR_INVALID_ARG;  // one plan = one device (create one per device)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return E3_ERR_NO_DEVICE;
  int32_t* d = nullptr;
  TpPath* dpaths = nullptr;
  auto fail = [&](int st) {
    if (d) (void)hipFree(d);
    if (dpaths) (void)hipFree(dpaths);
    fast_free(&P->fast);
    return st;
  };
  if (hipMalloc((void**)&d, P->h_tables.size() * sizeof(int32_t)) != hipSuccess) return fail(E3_ERR_HIP);
  if (hipMemcpy(d, P->h_tables.data(), P->h_tables.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    return fail(E3_ERR_HIP);
  const size_t np = std::max<size_t>(P->h_paths.size(), 1);
  if (hipMalloc((void**)&dpaths, np * sizeof(TpPath)) != hipSuccess) return fail(E3_ERR_HIP);
  if (!P->h_paths.empty() &&
      hipMemcpy(dpaths, P->h_paths.data(), P->h_paths.size() * sizeof(TpPath), hipMemcpyHostToDevice) != hipSuccess)
    return fail(E3_ERR_HIP);
  const int st = fast_upload(&P->fast);
  if (st != E3_OK) return fail(st);
  P->d_paths = dpaths;
  P->dev.cpos = d;
  P->dev.ocol = d + P->dev.D1;
  P->dev.paths = dpaths;
  P->device = cur;
  P->d_tables = d;
  return E3_OK;
}

// the MFMA section of a packed buffer: behind the fp32 generic section, 256-byte aligned (e3_tp_packed_bytes)
static const char* fast_section(const e3_tp_plan* p, const void* packed) {
  return (const char*)packed + ((p->dev.packed_elems + 64) * 4 + 255) / 256 * 256;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_tp_plan_create(const int32_t* in1_blocks, int n_in1, int lmax_sh, const int32_t* out_blocks, int n_out,
                      e3_tp_plan** plan_out) {
  if (!in1_blocks || !out_blocks || n_in1 <= 0 || n_out <= 0 || !plan_out) return E3_ERR_INVALID_ARG;
  if (lmax_sh < 1 || lmax_sh > 2) return E3_ERR_BAD_IRREPS;
  auto* P = new e3_tp_plan();
  TpDev& d = P->dev;
  d.lmax_sh = lmax_sh;
  d.Dy = (lmax_sh + 1) * (lmax_sh + 1);
  for (int c = 0; c < 6; ++c) d.n[c] = d.M[c] = 0;
  struct Blk { int l, p, mul, col; };
  std::vector<Blk> bi, bo;
  auto parse = [&](const int32_t* b, int n, std::vector<Blk>& v, int* dim) {
    int col = 0;
    for (int i = 0; i < n; ++i) {
      int l = b[3 * i], p = b[3 * i + 1], mul = b[3 * i + 2];
      if (l < 0 || l > 2 || (p != 1 && p != -1) || mul < 0) return false;
      v.push_back({l, p, mul, col});
      col += (2 * l + 1) * mul;
    }
    *dim = col;
    return true;
  };
  if (!parse(in1_blocks, n_in1, bi, &d.D1) || !parse(out_blocks, n_out, bo, &d.Dout)) {
    delete P;
    return E3_ERR_BAD_IRREPS;
  }
  auto cls = [](int l, int p) { return 2 * l + (p == 1 ? 0 : 1); };
  for (auto& b : bi) d.n[cls(b.l, b.p)] += b.mul;
  for (auto& b : bo) d.M[cls(b.l, b.p)] += b.mul;
  int pos = 0;
  for (int c = 0; c < 6; ++c) { d.cbase[c] = pos; pos += d.n[c] * (2 * (c >> 1) + 1); }
  pos = 0;
  for (int c = 0; c < 6; ++c) { d.obase[c] = pos; pos += d.M[c] * (2 * (c >> 1) + 1); }
  std::vector<int32_t> tables(d.D1, 0);
  {
    int fill[6] = {0, 0, 0, 0, 0, 0};
    for (auto& b : bi) {
      int c = cls(b.l, b.p), w = 2 * b.l + 1;
      for (int i = 0; i < b.mul * w; ++i) tables[b.col + i] = d.cbase[c] + fill[c] + i;
      fill[c] += b.mul * w;
    }
  }
  int off = 0;
  for (int c = 0; c < 6; ++c) {
    d.ocol_off[c] = off;
    for (auto& b : bo)
      if (cls(b.l, b.p) == c)
        for (int i = 0; i < b.mul; ++i) tables.push_back(b.col + i * (2 * b.l + 1));
    off += d.M[c];
  }
  tables.push_back(0);
  P->h_tables = std::move(tables);
  // paths per out class, ordered by (l1, l2)
  int64_t wpos = 0;
  for (int c3 = 0; c3 < 6; ++c3) {
    const int l3 = c3 >> 1, p3 = (c3 & 1) ? -1 : 1;
    d.poff[c3] = (int)P->h_paths.size();
    d.npath[c3] = 0;
    int wrow = 0;
    for (int l1 = 0; l1 <= 2; ++l1)
      for (int l2 = 0; l2 <= lmax_sh; ++l2) {
        if (l3 < std::abs(l1 - l2) || l3 > l1 + l2) continue;
        const int p2 = (l2 & 1) ? -1 : 1;
        const int c1 = cls(l1, p3 * p2);
        if (d.n[c1] == 0) continue;
        if (d.M[c3] > 0) {
          P->h_paths.push_back({c1, l1, l2, wrow});
          d.npath[c3]++;
        }
        wrow += d.n[c1];
      }
    d.K[c3] = d.M[c3] > 0 ? wrow : 0;
    d.woff[c3] = wpos;
    wpos += (int64_t)d.K[c3] * d.M[c3];
  }
  d.normcol_off = wpos;
  d.packed_elems = wpos + d.Dout;
  {
    std::vector<std::array<int, 4>> blocks;
    for (auto& b : bi) blocks.push_back({b.l, b.p, b.mul, b.col});
    std::vector<TpPath> by_class[6];
    for (int c3 = 0; c3 < 6; ++c3)
      for (int i = 0; i < d.npath[c3]; ++i) by_class[c3].push_back(P->h_paths[d.poff[c3] + i]);
    fast_plan_init(&P->fast, d.n, d.M, lmax_sh, d.Dout, d.Dy, blocks, by_class, d.ocol_off);
    // fused gate epilogue: every natural-parity out class must be one contiguous run of columns, in class order
    {
      bool ok = true;
      int expect = 0;
      for (int c : {0, 3, 4}) {
        const int w = 2 * (c >> 1) + 1;
        for (int i = 0; i < d.M[c]; ++i) ok = ok && P->h_tables[d.D1 + d.ocol_off[c] + i] == expect + i * w;
        expect += d.M[c] * w;
      }
      P->fast.gate_layout = ok;
    }
  }
  *plan_out = P;
  return E3_OK;
}

int e3_tp_plan_destroy(e3_tp_plan* P) {
  if (!P) return E3_OK;
  if (P->d_tables) (void)hipFree(P->d_tables);
  if (P->d_paths) (void)hipFree(P->d_paths);
  fast_free(&P->fast);
  delete P;
  return E3_OK;
}

int e3_tp_in1_dim(const e3_tp_plan* p) { return p ? p->dev.D1 : -1; }
int e3_tp_in2_dim(const e3_tp_plan* p) { return p ? p->dev.Dy : -1; }
int e3_tp_out_dim(const e3_tp_plan* p) { return p ? p->dev.Dout : -1; }
int e3_tp_weight_shape(const e3_tp_plan* p, int cls, int* rows, int* cols) {
  if (!p || cls < 0 || cls > 5 || !rows || !cols) return E3_ERR_INVALID_ARG;
  bool present = p->dev.K[cls] > 0 && p->dev.M[cls] > 0;
  *rows = present ? p->dev.K[cls] : 0;
  *cols = present ? p->dev.M[cls] : 0;
  return E3_OK;
}
int e3_tp_norm_len(const e3_tp_plan* p, int cls) {
  return (p && cls >= 0 && cls < 6) ? p->dev.M[cls] * (2 * (cls >> 1) + 1) : -1;
}
int64_t e3_tp_packed_bytes(const e3_tp_plan* p, int dtype) {
  if (!p || dtype < 0 || dtype > 2) return -1;
  int64_t b = ((p->dev.packed_elems + 64) * (dtype == E3_F64 ? 8 : 4) + 255) / 256 * 256;
  if (dtype != E3_F64) b += fast_packed_bytes(&p->fast);
  return b;
}

int e3_tp_pack_weights(const e3_tp_plan* plan, const void* const w[6], const void* const n[6], int dtype, void* packed,
                       void* stream) {
  if (!plan || !w || !packed || dtype < 0 || dtype > 2) return E3_ERR_INVALID_ARG;
  for (int c = 0; c < 6; ++c)
    if (plan->dev.M[c] > 0 && plan->dev.K[c] > 0 && !w[c]) return E3_ERR_MISSING_WEIGHT;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  TpPtr6 ww, nn;
  for (int c = 0; c < 6; ++c) {
    ww.p[c] = const_cast<void*>(w[c]);
    nn.p[c] = (n && plan->dev.M[c] > 0) ? const_cast<void*>(n[c]) : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  auto pack = [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(tp_pack_kernel<T>, dim3(64), dim3(256), 0, s, ww, nn, (typename AccOf<T>::type*)packed, plan->dev);
    E3_HIP_CHECK(hipGetLastError());
    return E3_OK;
  };
  st = dtype == E3_BF16 ? pack(TpTag<bf16>{}) : tp_by_dtype(dtype, pack);
  if (st != E3_OK) return st;
  if (dtype != E3_F64 && plan->fast.usable)
    return fast_pack(&plan->fast, w, nn.p, dtype, const_cast<char*>(fast_section(plan, packed)), plan->dev.ocol, s);
  return E3_OK;
}

int e3_tp_forward(const e3_tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                  const void* packed, void* out, int64_t ldo, int64_t B, int dtype, const float* in_scale, int exact,
                  void* stream) {
  if (!plan || B < 0 || dtype < 0 || dtype > 2) return E3_ERR_INVALID_ARG;
  if (B == 0) return E3_OK;
  if (!in1 || !in2 || !packed || !out) return E3_ERR_INVALID_ARG;
  if (dtype == E3_BF16 && (!plan->fast.usable || ld2 == 0)) return E3_ERR_UNSUPPORTED;  // bf16 storage: MFMA path only
  if (!tp_rows_ok(plan->dev, ld1, ld2, true, ldo)) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == E3_BF16 && exact) return E3_ERR_UNSUPPORTED;
  if (dtype != E3_F64 && plan->fast.usable && ld2 != 0 && !exact) {
    e3_tp_segment seg = {in1, ld1, nullptr, plan->dev.D1, 0};
    return fast_forward(&plan->fast, &seg, 1, plan->dev.D1, in2, ld2, fast_section(plan, packed), out, ldo, B, 0, dtype,
                        plan->dev.ocol, in_scale, s);
  }
  return tp_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int R = 16;
    const size_t lds = (size_t)R * (plan->dev.D1 + plan->dev.Dy) * sizeof(typename AccOf<T>::type);
    return tp_launch(tp_fwd_generic_kernel<T, R>, R, 256 * 8, lds, B, s, in1, ld1, in2, ld2, packed, out, ldo, B, plan->dev);
  });
}

int e3_tp_forward_fused(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg, const void* in2, int64_t ld2,
                        const void* packed, void* out, int64_t ldo, int64_t B, int dtype, int gate,
                        const float* in_scale, void* stream) {
  if (!plan || !segs || B < 0) return E3_ERR_INVALID_ARG;
  if ((dtype != E3_F32 && dtype != E3_BF16) || !plan->fast.usable || ld2 == 0) return E3_ERR_UNSUPPORTED;
  if (B == 0) return E3_OK;
  if (!in2 || !packed || !out || ld2 < plan->dev.Dy) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  return fast_forward(&plan->fast, segs, nseg, plan->dev.D1, in2, ld2, fast_section(plan, packed), out, ldo, B, gate, dtype,
                      plan->dev.ocol, in_scale, (hipStream_t)stream);
}

int e3_tp_forward_fused_epilogue(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg, const void* in2,
                                 int64_t ld2, const void* packed, void* out, int64_t ldo, int64_t B, int dtype, int gate,
                                 const float* in_scale, const void* residual, int64_t ld_residual, float* out_scale4,
                                 int target_log2, void* stream) {
  if (!plan || !segs || B < 0 || (residual && ld_residual <= 0)) return E3_ERR_INVALID_ARG;
  if (!tp_scale_arg_ok(out_scale4, target_log2)) return E3_ERR_INVALID_ARG;
  if ((dtype != E3_F32 && dtype != E3_BF16) || !plan->fast.usable || ld2 == 0) return E3_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* amax = nullptr;
  int st = tp_scale_begin(out_scale4, s, &amax);
  if (st != E3_OK) return st;
  if (B > 0) {
    if (!in2 || !packed || !out || ld2 < plan->dev.Dy) return E3_ERR_INVALID_ARG;
    st = tp_ensure_device(plan);
    if (st != E3_OK) return st;
    st = fast_forward(&plan->fast, segs, nseg, plan->dev.D1, in2, ld2, fast_section(plan, packed), out, ldo, B, gate, dtype,
                      plan->dev.ocol, in_scale, s, nullptr, residual, ld_residual, amax);
    if (st != E3_OK) return st;
  }
  return tp_scale_end(out_scale4, target_log2, s);
}

int e3_tp_forward_update_pair(const e3_tp_plan* plan1, const e3_tp_plan* plan2, const e3_tp_segment* segs, int nseg,
                              const void* in2, int64_t ld2, const void* packed1, const void* packed2,
                              const float* in_scale, const void* residual, int64_t ld_residual, void* out, int64_t ldo,
                              int64_t B, int dtype, float* out_scale4, int target_log2, void* stream) {
  if (!plan1 || !plan2 || !segs || B < 0 || (residual && ld_residual <= 0)) return E3_ERR_INVALID_ARG;
  if (!tp_scale_arg_ok(out_scale4, target_log2)) return E3_ERR_INVALID_ARG;
  if ((dtype != E3_F32 && dtype != E3_BF16) || ld2 == 0 || !e3::r16_pair_supported(&plan1->fast, &plan2->fast))
    return E3_ERR_UNSUPPORTED;
  if (!in2 || !packed1 || !packed2 || !out || ld2 < plan1->dev.Dy || ldo < plan2->dev.Dout) return E3_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  int st = tp_ensure_device(plan1);
  if (st == E3_OK) st = tp_ensure_device(plan2);
  if (st != E3_OK) return st;
  uint32_t* amax = nullptr;
  st = tp_scale_begin(out_scale4, s, &amax);
  if (st != E3_OK) return st;
  if (B > 0) {
    st = fast_forward_pair(&plan1->fast, &plan2->fast, segs, nseg, plan1->dev.D1, in2, ld2, fast_section(plan1, packed1),
                           fast_section(plan2, packed2), out, ldo, B, dtype, plan1->dev.ocol, plan2->dev.ocol, in_scale,
                           residual, ld_residual, amax, s);
    if (st != E3_OK) return st;
  }
  return tp_scale_end(out_scale4, target_log2, s);
}

int e3_tp_forward_fused_scatter(const e3_tp_plan* plan, const e3_tp_segment* segs, int nseg, const void* in2,
                                int64_t ld2, const void* packed, const int32_t* row_node, void* out_nodes,
                                int64_t ldo, int64_t B, int dtype, int gate, const float* in_scale, void* stream) {
  if (!plan || !segs || !row_node || B < 0) return E3_ERR_INVALID_ARG;
  if ((dtype != E3_F32 && dtype != E3_BF16) || !gate || !plan->fast.usable || ld2 == 0) return E3_ERR_UNSUPPORTED;
  if (B == 0) return E3_OK;
  if (!in2 || !packed || !out_nodes || ld2 < plan->dev.Dy) return E3_ERR_INVALID_ARG;
  int st = tp_ensure_device(plan);
  if (st != E3_OK) return st;
  return fast_forward(&plan->fast, segs, nseg, plan->dev.D1, in2, ld2, fast_section(plan, packed), out_nodes, ldo, B, gate,
                      dtype, plan->dev.ocol, in_scale, (hipStream_t)stream, row_node);
}

const char* e3_tp_last_fused_kernel(void) { return fast_last_kernel(); }

int e3_tp_fused_supported(const e3_tp_plan* plan, int gate) {
  if (!plan || !plan->fast.usable) return 0;
  if (!gate) return 1;
  if (!plan->fast.gate_layout) return 0;
  return e3::fast_gate_shape_ok(&plan->fast) ? 1 : 0;
}

}  // extern "C"
