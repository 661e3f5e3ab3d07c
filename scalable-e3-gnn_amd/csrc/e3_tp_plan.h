// General SH tensor product: the plan and the host helpers its three sources share (e3_tp.hip: plan, pack, forward entries;
// e3_tp_bwd.hip: generic backward; e3_tp_wgrad.hip: fp32-MFMA weight gradient).
#pragma once
#include "e3_common.h"
#include "e3_tp_internal.h"

#include <algorithm>

namespace e3 {

struct TpDev {
  int D1, Dout, Dy, lmax_sh;
  int n[6], M[6], cbase[6], obase[6], ocol_off[6], npath[6], poff[6], K[6];
  int64_t woff[6];
  int64_t normcol_off, packed_elems;
  const int32_t* cpos;
  const int32_t* ocol;
  const TpPath* paths;
};

struct TpPtr6 { void* p[6]; };  // one pointer per class, as a kernel argument

}  // namespace e3

struct e3_tp_plan {
  e3::TpDev dev;
  std::vector<int32_t> h_tables;  // [cpos (D1) | ocol (sum M)]
  std::vector<e3::TpPath> h_paths;
  int32_t* d_tables = nullptr;
  e3::TpPath* d_paths = nullptr;
  e3::TpFast fast;
  std::mutex mu;
  int device = -1;  // the device the tables were uploaded to (the one current at first use); calls from another one fail
};

namespace e3 {

// uploads the plan's tables on first use (e3_tp.hip); E3_ERR_INVALID_ARG from a device other than the plan's
int tp_ensure_device(const e3_tp_plan* plan);

constexpr int kTpThreads = 256;  // workgroup size of every generic kernel (their loops stride by it)

// One launch of a row-tiled kernel with dynamic LDS: refused above 160 KB, the function's limit raised, one workgroup per
// `rows` rows up to `grid_cap`.  The arguments are converted to the kernel's parameter types (void* -> typed pointers).
template <typename... P, typename... Args>
inline int tp_launch(void (*kern)(P...), int rows, int grid_cap, size_t lds, int64_t B, hipStream_t s, const Args&... args) {
  if (lds > 160 * 1024) return E3_ERR_UNSUPPORTED;
  if (const int st = ensure_dyn_lds((const void*)kern, lds); st != E3_OK) return st;
  const int grid = (int)std::min<int64_t>((B + rows - 1) / rows, grid_cap);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kTpThreads), lds, s, (P)args...);
  E3_HIP_CHECK(hipGetLastError());
  return E3_OK;
}

// f(TpTag<float>) for E3_F32, f(TpTag<double>) otherwise (the entries have refused every other dtype before)
template <typename T> struct TpTag { using type = T; };
template <typename F>
inline int tp_by_dtype(int dtype, F&& f) { return dtype == E3_F32 ? f(TpTag<float>{}) : f(TpTag<double>{}); }

// ---- argument checks shared by the entries (each failure is E3_ERR_INVALID_ARG at the place the entry calls it) ----
// leading dimensions of the in rows: in1, in2 (ld2 = 0: one broadcast row) and, with `has_o`, the Dout-wide out / grad_out rows
inline bool tp_rows_ok(const TpDev& p, int64_t ld1, int64_t ld2, bool has_o, int64_t ldo) {
  return ld1 >= p.D1 && (!has_o || ldo >= p.Dout) && (ld2 == 0 || ld2 >= p.Dy);
}
// leading dimensions of the requested operand gradients; a broadcast in2 has a one-row gradient and vice versa
inline bool tp_grad_rows_ok(const TpDev& p, const void* gin1, int64_t ldg1, const void* gin2, int64_t ldg2, int64_t ld2) {
  if (gin1 && ldg1 < p.D1) return false;
  return !gin2 || ((ld2 == 0) == (ldg2 == 0) && (ldg2 == 0 || ldg2 >= p.Dy));
}
// out_scale4 of the epilogue entries (NULL = not wanted): its range check, then begin / end around the launch.  begin
// zeroes the four words on the stream and yields the word the kernels' atomic max goes to; end derives {s, 1 / s} from it
inline bool tp_scale_arg_ok(const float* out_scale4, int target_log2) {
  return !out_scale4 || (target_log2 >= -20 && target_log2 <= 14);
}
inline int tp_scale_begin(float* out_scale4, hipStream_t s, uint32_t** amax) {
  *amax = out_scale4 ? reinterpret_cast<uint32_t*>(out_scale4) + 2 : nullptr;
  if (out_scale4) E3_HIP_CHECK(hipMemsetAsync(out_scale4, 0, 16, s));
  return E3_OK;
}
inline int tp_scale_end(float* out_scale4, int target_log2, hipStream_t s) {
  return out_scale4 ? scale_finalize(out_scale4, target_log2, s) : E3_OK;
}

}  // namespace e3
