// L1 tensor product (the pinned operator): its class table, its plan and the host helpers its three sources share
// (e3_l1tp.hip: plan, generic pack and forward, ABI entries; e3_l1tp_bwd.hip: generic backward; e3_l1tp_mfma.hip: fp32 MFMA
// forward).  Reference semantics: the reference's models/segnn/l1_tensor_prod.py, cited as L1TP.py:<line>.
#pragma once
#include "e3_common.h"

namespace e3 {

constexpr double kC3 = 0.57735026918962576451;  // 1/sqrt(3)  cg110 = cg011, L1TP.py:92-93
constexpr double kC6 = 0.40824829046386301637;  // 1/sqrt(6)  cg111,         L1TP.py:94

constexpr int kL1LdsBudget = 160 * 1024;  // dynamic LDS a launch of this family may ask for

// ---- the class table ------------------------------------------------------------------------------------------------
// Classes are 0e, 0o, 1e, 1o = 0 .. 3.  kL1Src[out class][slot] = the input class whose channels form that block of the out
// class's weight rows, in weight-row order (L1TP.py:81-88); -1 = no such block.  Slots: 0 = scalars (x Y0 for a scalar
// output, (x) Y1 for a vector output), 1 = vectors dotted with Y1 (scalar output) or taken with Y0 (vector output),
// 2 = vectors crossed with Y1 (vector outputs only).
constexpr int kL1Src[4][3] = {{0, 3, -1}, {1, 2, -1}, {1, 2, 3}, {0, 3, 2}};
// The inverse view: kL1Dst[in class][j] = the output class that consumes the input class as its block of slot
// l1_dst_slot(in, j); j = 0: the scalar output, 1: the vector output it reaches without a cross product, 2: with one.  The
// two tables have the same entries: the operator is its own dual (what L1TensorProduct._dual_forward runs on).
constexpr int kL1Dst[4][3] = {{0, 3, -1}, {1, 2, -1}, {1, 2, 3}, {0, 3, 2}};
__host__ __device__ constexpr int l1_dst_slot(int in, int j) { return in < 2 ? 0 : (j == 2 ? 2 : 1); }

constexpr bool l1_tables_inverse() {  // every (in, j) names a block that holds `in`, twice never, and none is left over
  int nsrc = 0, ndst = 0;
  for (int c = 0; c < 4; ++c)
    for (int j = 0; j < 3; ++j) {
      nsrc += kL1Src[c][j] >= 0;
      const int o = kL1Dst[c][j];
      if (o < 0) continue;
      ++ndst;
      if (kL1Src[o][l1_dst_slot(c, j)] != c) return false;
      for (int i = 0; i < j; ++i)
        if (kL1Dst[c][i] == o && l1_dst_slot(c, i) == l1_dst_slot(c, j)) return false;
    }
  return nsrc == ndst;
}
static_assert(l1_tables_inverse(), "kL1Dst is not the inverse of kL1Src");

// first weight row of `slot` in the matrix of out class c: the channel counts n[] of the earlier slots (slot = 3: all rows)
__host__ __device__ constexpr int l1_wrow(const int* n, int c, int slot) {
  int r = 0;
  for (int s = 0; s < slot; ++s)
    if (kL1Src[c][s] >= 0) r += n[kL1Src[c][s]];
  return r;
}

// ---- irreps bookkeeping (host) --------------------------------------------------------------------------------------
struct Block {  // one `mul x (l,p)` entry of an Irreps, with its first column
  int l, p, mul, col;
};

// One contiguous run of channels of a class inside a row: channel i of the run starts at column
// col + i*cstride (cstride = 1 for scalars, 3 for vectors whose 3 components are adjacent).
struct Run {
  int col, count, cstride;
};

// Device-visible plan (POD, passed by value as a kernel argument).
struct PlanDev {
  int D1, Dout;
  int n[4];          // in1 channel counts per class: n0e, n0o, n1e, n1o
  int M[4];          // out multiplicities per class
  int cbase[4];      // first canonical position of class c inside a staged in1 row
  int obase[4];      // first canonical position of class c inside a staged out / grad_out row
  int icol_off[4];   // offset of class c inside `icol`
  int ocol_off[4];   // offset of class c inside `ocol`
  const int32_t* cpos;  // [D1]   in1 column -> canonical position ([s0e|s0o|v1e|v1o], xyz adjacent)
  const int32_t* opos;  // [Dout] out column -> canonical position (same class order)
  const int32_t* icol;  // [sum n] first in1 column of channel k of class c
  const int32_t* ocol;  // [sum M] first out column of channel m of class c
};

template <typename T> struct L1Ptr4 { T* p[4]; };  // one pointer per class, as a kernel argument
template <typename T>
inline L1Ptr4<T> l1_ptr4(const void* const v[4]) {  // NULL array = four NULLs
  L1Ptr4<T> r;
  for (int c = 0; c < 4; ++c) r.p[c] = v ? (T*)v[c] : nullptr;
  return r;
}

struct Mfma;

}  // namespace e3

struct e3_l1tp_plan {
  std::vector<e3::Block> in1, out;
  std::vector<e3::Run> irun[4], orun[4];
  e3::PlanDev dev;
  std::vector<int32_t> h_tables;  // [cpos (D1) | opos (Dout) | icol (sum n) | ocol (sum M)]
  int32_t* d_tables = nullptr;    // uploaded on first use
  int device = -1;                // ... to the device current at that moment; calls from another device fail
  std::mutex mu;
  int wrows[4], wcols[4];
  int normlen[4];
  // MFMA path (filled by mfma_plan_init)
  e3::Mfma* mfma = nullptr;
};

namespace e3 {

// uploads the plan's tables on first use (e3_l1tp.hip); E3_ERR_INVALID_ARG from a device other than the plan's
int ensure_device(const e3_l1tp_plan* plan);

// mfma path (e3_l1tp_mfma.hip)
int mfma_plan_init(e3_l1tp_plan* plan);    // host only
int mfma_plan_upload(e3_l1tp_plan* plan);  // device tables
void mfma_plan_free(e3_l1tp_plan* plan);
bool mfma_supported(const e3_l1tp_plan* plan, int dtype);
int64_t mfma_packed_bytes(const e3_l1tp_plan* plan);
int mfma_pack(const e3_l1tp_plan* plan, const void* const weights[4], const void* const norms[4], int dtype,
              void* packed, hipStream_t stream);
int mfma_forward(const e3_l1tp_plan* plan, const void* in1, int64_t ld1, const void* in2, int64_t ld2,
                 const void* packed, void* out, int64_t ldo, int64_t B, int dtype, hipStream_t stream);

// Packed buffer, section 1 (all dtypes): [W0e | W0o | W1e | W1o | normcol[Dout]] in the accumulate type; section 2 (MFMA
// tiles, fp32 and bf16 storage) follows at a 256-byte aligned offset.
struct PackOffsets {
  int64_t w[4];
  int64_t normcol;
  int64_t end;  // elements
};
inline PackOffsets pack_offsets(const e3_l1tp_plan* p) {
  PackOffsets o;
  int64_t pos = 0;
  for (int c = 0; c < 4; ++c) {
    o.w[c] = pos;
    pos += (int64_t)p->wrows[c] * p->wcols[c];
  }
  o.normcol = pos;
  pos += p->dev.Dout;
  o.end = (pos + 63) / 64 * 64;
  return o;
}
inline size_t l1_acc_size(int dtype) { return dtype == E3_F64 ? 8 : 4; }
inline int64_t l1_mfma_section_offset(const e3_l1tp_plan* p, int dtype) {  // bytes
  return (pack_offsets(p).end * (int64_t)l1_acc_size(dtype) + 255) / 256 * 256;
}

// f(L1Tag<float>) for E3_F32, f(L1Tag<double>) for E3_F64, f(L1Tag<bf16>) otherwise (the entries have refused every other
// dtype before)
template <typename T> struct L1Tag { using type = T; };
template <typename F>
inline int l1_by_dtype(int dtype, F&& f) {
  return dtype == E3_F32 ? f(L1Tag<float>{}) : dtype == E3_F64 ? f(L1Tag<double>{}) : f(L1Tag<bf16>{});
}

}  // namespace e3
