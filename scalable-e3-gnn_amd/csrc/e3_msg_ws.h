// Weights-stationary form of the fused message kernel (e3_msg_ws.hip); launched by e3_msg_forward (e3_msg_fused.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace e3 {
struct PbcCell;
bool msg_ws_supported(int lmax, int hidden, int dtype);
// floats per node of the pre-split rows the fp32 kernel gathers (MsgSplit, e3_msg_common.h); 0: the shape never takes this kernel
int msg_ws_split_floats(int lmax, int hidden);
// Same operands as e3_msg_forward after its checks; `out` already zeroed (or holding the sums to continue).  chunk_edges:
// edges per chunk of the workgroups' round-robin (0 = default 256).  `premix` = what e3_msg_premix wrote: N table rows, the N pre-split
// rows, then the N per-node row maxima of h * in_scale (msg_premix_layout).  `box` (host, 3 floats: L per axis, 0 = open; NULL = open box): the periodic
// instantiation with the minimum image of e3_msg_forward_pbc.  `cell` (what make_cell derived; excludes `box`): the cell instantiation
// of e3_msg_forward_cell.
int msg_ws_launch(int lmax, int hidden, int dtype, const void* h, int64_t ldh, int64_t N, const float* pos4, const int32_t* src,
                  const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix, float* out,
                  int64_t ldo, int chunk_edges, hipStream_t stream, const float* box = nullptr,
                  const PbcCell* cell = nullptr);
}  // namespace e3
