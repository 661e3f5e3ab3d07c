// Plans and packed weights of the SEGNN message function (e3_msg_plan_*, e3_msg_pack_weights; include/e3gnn.h), host side:
// the weight blocks of both products in MFMA A-operand order, as fp16 (hi, lo) halves scaled by a power of two (fp32
// storage) or as bf16, with the norm tables, the d-term weights and the header the edge kernels read.  The packing kernels
// are compiled with the fp32 edge kernels (msg_pack_launch, e3_msg_fused_f32.hip, which says why).
#include "e3_msg_plan.h"
#include "cg_tables.h"

#include <algorithm>

namespace e3 {
#include "e3_tp_mfma_core.h"
#include "e3_msg_common.h"

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
template <int LMAX, int TT>
static MsgShape make_shape(int index) {
  using G = MsgGeom<LMAX, TT>;
  return {index, LMAX, TT, TT >= 2, G::total_floats, G::UD, G::D, G::lds_tab, G::lds_wave, G::nblk(), G::NS, G::WD,
          G::o_norm1, G::o_norm2, G::o_wd, G::o_w};
}
#define E3_MSG_SHAPE_ENTRY(I, LMAX, TT) make_shape<LMAX, TT>(I),
static const MsgShape kShapes[kMsgShapes] = {E3_MSG_SHAPES(E3_MSG_SHAPE_ENTRY)};
#undef E3_MSG_SHAPE_ENTRY

int msg_ensure_device(e3_msg_plan* P) {
  std::lock_guard<std::mutex> lock(P->mu);
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return E3_ERR_NO_DEVICE;
  if (P->d_desc) return cur == P->device ? E3_OK : E3_ERR_INVALID_ARG;
  MsgPackDesc* d = nullptr;
  E3_HIP_CHECK(hipMalloc((void**)&d, P->desc.size() * sizeof(MsgPackDesc)));
  if (hipMemcpy(d, P->desc.data(), P->desc.size() * sizeof(MsgPackDesc), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return E3_ERR_HIP;
  }
  for (int io = 0; io < (P->k->bf16 ? 2 : 1); ++io)
    for (PbcMode mode : {kOpen, kBox}) {
      if (msg_fused_setup(*P->k, mode, io, cur, nullptr) != E3_OK) {
        (void)hipFree(d);
        return E3_ERR_HIP;
      }
    }
  P->device = cur;
  P->d_desc = d;
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_msg_plan_create(int lmax, int hidden, e3_msg_plan** plan_out) {
  if (!plan_out || lmax < 1 || lmax > 2) return E3_ERR_INVALID_ARG;
  const MsgShape* k = nullptr;
  for (auto& e : kShapes)
    if (e.lmax == lmax && 16 * e.tt == hidden) k = &e;
  if (!k) return E3_ERR_UNSUPPORTED;  // hidden in {16, 32, 64}
  auto* P = new e3_msg_plan();
  P->lmax = lmax; P->H = hidden; P->k = k;
  const int H = hidden, TT = k->tt, KS = (H + 31) / 32;
  auto ok = [&](int l1, int l2, int l3) {
    return l1 <= lmax && l2 <= lmax && l3 <= lmax && ((l1 + l2 + l3) % 2 == 0) && l3 >= std::abs(l1 - l2) && l3 <= l1 + l2;
  };
  auto T = [&](int l3) { return l3 == 0 ? TT * (1 + lmax) : TT; };
  // class-matrix row offsets: paths ordered by (l1, l2) ascending (e3_tp_plan_create), n rows each
  const int n1[3] = {2 * H + 1, 2 * H, 2 * H}, n2[3] = {H, H, H};
  int wrow1[3][3][3], wrow2[3][3][3];
  for (int l3 = 0; l3 <= 2; ++l3) {
    int r1 = 0, r2 = 0;
    for (int l1 = 0; l1 <= 2; ++l1)
      for (int l2 = 0; l2 <= 2; ++l2) {
        wrow1[l1][l2][l3] = wrow2[l1][l2][l3] = -1;
        if (l3 > lmax || !ok(l1, l2, l3)) continue;
        wrow1[l1][l2][l3] = r1; r1 += n1[l1];
        wrow2[l1][l2][l3] = r2; r2 += n2[l1];
      }
    P->K1[l3] = l3 <= lmax ? r1 : 0;
    P->K2[l3] = l3 <= lmax ? r2 : 0;
    P->M[l3] = l3 <= lmax ? 16 * T(l3) : 0;
    P->rowd[l3] = (l3 <= lmax) ? wrow1[0][l3][l3] + 2 * H : 0;
  }
  // blocks in the kernels' order: l1 outer, then l3, then l2; (ks, t) inside a path
  int b = 0;
  for (int l1 = 0; l1 <= lmax; ++l1)
    for (int l3 = 0; l3 <= lmax; ++l3)
      for (int l2 = 0; l2 <= lmax; ++l2) {
        if (!ok(l1, l2, l3)) continue;
        for (int ks = 0; ks < KS; ++ks)
          for (int t = 0; t < T(l3); ++t) {
            const int nvalid = std::min(32, H - 32 * ks);
            const int M = 16 * T(l3);
            P->desc.push_back({0, l3, wrow1[l1][l2][l3] + H + 32 * ks, nvalid, M, 16 * t, b + ks * T(l3) + t});  // src rows
            P->desc.push_back({2, l3, wrow1[l1][l2][l3] + 32 * ks, nvalid, M, 16 * t, b + ks * T(l3) + t});      // dst rows
            P->desc.push_back({1, l3, wrow2[l1][l2][l3] + 32 * ks, nvalid, M, 16 * t, b + ks * T(l3) + t});
          }
        b += KS * T(l3);
      }
  if (b != k->nblk) { delete P; return E3_ERR_INVALID_ARG; }
  *plan_out = P;
  return E3_OK;
}

int e3_msg_plan_destroy(e3_msg_plan* P) {
  if (!P) return E3_OK;
  if (P->d_desc) (void)hipFree(P->d_desc);
  delete P;
  return E3_OK;
}

int64_t e3_msg_packed_bytes(const e3_msg_plan* P) { return P ? (P->k->total_floats * 4 + 255) / 256 * 256 : -1; }
int e3_msg_weight_shape(const e3_msg_plan* P, int tp, int l3, int* rows, int* cols) {
  if (!P || !rows || !cols || l3 < 0 || l3 > 2 || (tp != 1 && tp != 2)) return E3_ERR_INVALID_ARG;
  *rows = tp == 1 ? P->K1[l3] : P->K2[l3];
  *cols = P->M[l3];
  return E3_OK;
}

int e3_msg_supports(const e3_msg_plan* P, int dtype) {
  if (!P) return 0;
  return dtype == E3_F32 ? 1 : (dtype == E3_BF16 && P->k->bf16) ? 1 : 0;
}

int e3_msg_pack_weights(e3_msg_plan* P, const void* const w1[3], const void* const n1[3], const void* const w2[3],
                        const void* const n2[3], int dtype, void* packed, void* stream) {
  if (!P || !w1 || !w2 || !packed) return E3_ERR_INVALID_ARG;
  if (!e3_msg_supports(P, dtype)) return E3_ERR_UNSUPPORTED;
  for (int l = 0; l <= P->lmax; ++l)
    if (!w1[l] || !w2[l]) return E3_ERR_MISSING_WEIGHT;
  int st = msg_ensure_device(P);
  if (st != E3_OK) return st;
  const MsgShape& k = *P->k;
  MsgPackArgs a;
  for (int l = 0; l < 3; ++l) {
    const bool on = l <= P->lmax;
    a.w1[l] = on ? w1[l] : nullptr; a.w2[l] = on ? w2[l] : nullptr;
    a.n1[l] = (on && n1) ? n1[l] : nullptr; a.n2[l] = (on && n2) ? n2[l] : nullptr;
    a.nw1[l] = on ? (int64_t)P->K1[l] * P->M[l] : 0;
    a.nw2[l] = on ? (int64_t)P->K2[l] * P->M[l] : 0;
    a.rowd[l] = P->rowd[l];
  }
  a.M0 = P->M[0]; a.H = P->H; a.LMAX = P->lmax; a.TT = k.tt; a.NS = k.NS; a.WD = k.WD;
  a.o_norm1 = k.o_norm1; a.o_norm2 = k.o_norm2; a.o_wd = k.o_wd; a.o_w = k.o_w; a.nblk = k.nblk;
  return msg_pack_launch(a, P->d_desc, (int)P->desc.size(), dtype, packed, (hipStream_t)stream);
}

}  // extern "C"
