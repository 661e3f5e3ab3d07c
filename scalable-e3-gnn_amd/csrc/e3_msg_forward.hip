// The six e3_msg_forward* entries (include/e3gnn.h): argument checks, the choice between the two edge kernels
// (e3_msg_ws.hip: weights stationary, H = 32; e3_msg_fused.hip: one wave per tile, everything else) and the owned-sums
// orchestration.  Each entry builds the periodicity of the call once (MsgPbc) and hands the operands to msg_forward.
#include "e3_msg_plan.h"

using namespace e3;

// Owned sums (e3_msg_forward_owned*): the weights-stationary launch + the boundary merge and the isolated-rows kernel behind
// it (e3_msg_owned.hip) write every row of `out` exactly once (the ownership rule stands above `flush` in e3_msg_ws.hip).
// [part_node: 2 ints per chunk, padded to 256 bytes][part: 2 x D floats per chunk]
static int64_t owned_node_bytes(int64_t nchunks) { return (nchunks * 8 + 255) / 256 * 256; }
static int64_t owned_workspace_bytes(const e3_msg_plan* P, int64_t E, int dtype, int tiles_per_block) {
  if (!P || E < 0 || E > 0x7fffffffLL - 65536 || tiles_per_block < 0 || !msg_ws_supported(P->lmax, P->H, dtype)) return -1;
  if (E == 0) return 0;
  const int64_t nch = msg_ws_owned_chunks(E, tiles_per_block);
  return owned_node_bytes(nch) + nch * 2 * (int64_t)P->k->D * 4;
}

// owned != NULL: the owned-sums form (e3_msg_forward_owned*): no zero-fill, every row of `out` stored once, and the operand
// scale of `out` from the same launches; a.accumulate is 0 then.  Otherwise the sums arrive by atomics in an `out` that this
// function zeroes unless the call continues earlier sums (a.accumulate: sharded and continued launches).
static int msg_forward(e3_msg_plan* P, const MsgOperands& a, const MsgPbc& pbc, const MsgOwned* owned) {
  if (!P || a.N < 0 || a.E < 0 || a.E > 0x7fffffffLL - 16) return E3_ERR_INVALID_ARG;  // edge ids are int32
  if (!e3_msg_supports(P, a.dtype)) return E3_ERR_UNSUPPORTED;
  int64_t need = 0;
  if (owned) {
    if (a.accumulate || owned->target_log2 < -20 || owned->target_log2 > 14) return E3_ERR_INVALID_ARG;
    need = owned_workspace_bytes(P, a.E, a.dtype, a.tiles_per_block);
    if (need < 0) return E3_ERR_UNSUPPORTED;  // shapes of the one-wave-per-tile kernel: e3_msg_forward + e3_pow2_scale
    if (need > 0 && (!owned->workspace || owned->workspace_bytes < need || ((uintptr_t)owned->workspace & 15)))
      return E3_ERR_INVALID_ARG;
  }
  const MsgShape& k = *P->k;
  const int es = a.dtype == E3_BF16 ? 2 : 4;
  hipStream_t s = a.stream;
  if (a.N == 0) {
    if (owned) {
      E3_HIP_CHECK(hipMemsetAsync(owned->out_scale4, 0, 16, s));
      return scale_finalize(owned->out_scale4, owned->target_log2, s);
    }
    return E3_OK;
  }
  if (!a.h || !a.pos4 || !a.packed || !a.premix || !a.out || a.ld_h < k.D || a.ld_out < k.D || (a.E > 0 && (!a.src || !a.dst)))
    return E3_ERR_INVALID_ARG;
  if ((a.ld_h * es & 15) || ((uintptr_t)a.h & 15) || ((uintptr_t)a.premix & 15)) return E3_ERR_INVALID_ARG;  // 16-byte row gathers
  int st = msg_ensure_device(P);
  if (st != E3_OK) return st;
  // (owned sums with E > 0: every row is stored once by one of the three writers -- no fill)
  if (!a.accumulate && !(owned && a.E > 0))
    E3_HIP_CHECK(hipMemset2DAsync(a.out, (size_t)a.ld_out * 4, 0, (size_t)k.D * 4, (size_t)a.N, s));
  if (owned) {
    E3_HIP_CHECK(hipMemsetAsync(owned->out_scale4, 0, 16, s));
    if (a.E > 0) {
      const int64_t nch = msg_ws_owned_chunks(a.E, a.tiles_per_block);
      MsgWsOwned w;
      w.part_node = static_cast<int*>(owned->workspace);
      w.part = reinterpret_cast<float*>(static_cast<char*>(owned->workspace) + owned_node_bytes(nch));
      w.amax = reinterpret_cast<uint32_t*>(owned->out_scale4) + 2;
      E3_HIP_CHECK(hipMemsetAsync(w.part_node, 0xFF, (size_t)nch * 8, s));  // -1: slots that no chunk fills
      st = msg_ws_launch(*P, a, pbc, &w);
      if (st != E3_OK) return st;
      st = msg_owned_finish(w.part, w.part_node, 2 * nch, a.dst, a.E, a.N, k.D, a.out, a.ld_out, w.amax, s);
      if (st != E3_OK) return st;
    }
    return scale_finalize(owned->out_scale4, owned->target_log2, s);
  }
  if (a.E == 0) return E3_OK;
  // H = 32: the weights-stationary kernel; tiles_per_block > 0 = its chunk size in 16-edge units.  tiles_per_block < 0 asks
  // for the one-wave-per-tile kernel with |tiles_per_block| tiles per wave block.
  if (a.tiles_per_block >= 0 && msg_ws_supported(P->lmax, P->H, a.dtype)) {
    st = msg_ws_launch(*P, a, pbc, nullptr);
    if (st != E3_ERR_UNSUPPORTED) return st;
  }
  return msg_fused_launch(*P, a, pbc);
}

// the periodicity of a *_pbc / *_cell entry; false: a box or cell the entry rejects
static bool pbc_box(const float* box, MsgPbc* p) {
  if (!box_valid(box, 0.0f)) return false;
  p->mode = kBox;
  p->box = make_box(box);
  return true;
}
static bool pbc_cell(const float* cell, MsgPbc* p) {
  p->mode = kCell;
  return make_cell(cell, 0.0f, &p->cell);
}

extern "C" {

int e3_msg_forward(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                   const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                   float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block, void* stream) {
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, accumulate,
                         tiles_per_block, (hipStream_t)stream};
  return msg_forward(P, a, MsgPbc{}, nullptr);
}

int e3_msg_forward_pbc(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                       const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                       float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block, const float box[3],
                       void* stream) {
  MsgPbc pbc;
  if (!pbc_box(box, &pbc)) return E3_ERR_INVALID_ARG;
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, accumulate,
                         tiles_per_block, (hipStream_t)stream};
  return msg_forward(P, a, pbc, nullptr);
}

int e3_msg_forward_cell(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                        const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                        float* out, int64_t ld_out, int dtype, int accumulate, int tiles_per_block, const float cell[9],
                        void* stream) {
  MsgPbc pbc;
  if (!pbc_cell(cell, &pbc)) return E3_ERR_INVALID_ARG;
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, accumulate,
                         tiles_per_block, (hipStream_t)stream};
  return msg_forward(P, a, pbc, nullptr);
}

int64_t e3_msg_owned_workspace_bytes(const e3_msg_plan* P, int64_t E, int dtype, int tiles_per_block) {
  return owned_workspace_bytes(P, E, dtype, tiles_per_block);
}

int e3_msg_forward_owned(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                         const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                         float* out, int64_t ld_out, int dtype, int tiles_per_block, void* workspace,
                         int64_t workspace_bytes, float* out_scale4, int target_log2, void* stream) {
  if (!out_scale4) return E3_ERR_INVALID_ARG;
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, 0, tiles_per_block,
                         (hipStream_t)stream};
  const MsgOwned owned = {workspace, workspace_bytes, out_scale4, target_log2};
  return msg_forward(P, a, MsgPbc{}, &owned);
}

int e3_msg_forward_owned_pbc(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                             const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                             float* out, int64_t ld_out, int dtype, int tiles_per_block, void* workspace,
                             int64_t workspace_bytes, float* out_scale4, int target_log2, const float box[3], void* stream) {
  MsgPbc pbc;
  if (!out_scale4 || !pbc_box(box, &pbc)) return E3_ERR_INVALID_ARG;
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, 0, tiles_per_block,
                         (hipStream_t)stream};
  const MsgOwned owned = {workspace, workspace_bytes, out_scale4, target_log2};
  return msg_forward(P, a, pbc, &owned);
}

int e3_msg_forward_owned_cell(e3_msg_plan* P, const void* h, int64_t ld_h, int64_t N, const float* pos4, const int32_t* src,
                              const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix,
                              float* out, int64_t ld_out, int dtype, int tiles_per_block, void* workspace,
                              int64_t workspace_bytes, float* out_scale4, int target_log2, const float cell[9],
                              void* stream) {
  MsgPbc pbc;
  if (!out_scale4 || !pbc_cell(cell, &pbc)) return E3_ERR_INVALID_ARG;
  const MsgOperands a = {h, ld_h, N, pos4, src, dst, E, packed, in_scale, premix, out, ld_out, dtype, 0, tiles_per_block,
                         (hipStream_t)stream};
  const MsgOwned owned = {workspace, workspace_bytes, out_scale4, target_log2};
  return msg_forward(P, a, pbc, &owned);
}

}  // extern "C"
