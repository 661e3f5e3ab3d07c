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
// `part` (with `part_node`, `amax`; nullptr = sums by atomics into `out`): OWNED SUMS for a launch that does not accumulate.
// `out` needs no zero-fill: the kernel stores the rows whose run lies inside one chunk itself and joins their max |x| (finite
// values) into the max-bits word `amax`; the first and the last flushed node of chunk c leave their partial sums in
// part[2 c + {0, 1}][D] and their ids in part_node[2 c + {0, 1}] (preset to -1 by the caller; msg_ws_owned_chunks(E,
// chunk_edges) chunks, in edge order), for the boundary merge behind the launch.
int msg_ws_launch(int lmax, int hidden, int dtype, const void* h, int64_t ldh, int64_t N, const float* pos4, const int32_t* src,
                  const int32_t* dst, int64_t E, const void* packed, const float* in_scale, const float* premix, float* out,
                  int64_t ldo, int chunk_edges, hipStream_t stream, const float* box = nullptr,
                  const PbcCell* cell = nullptr, float* part = nullptr, int* part_node = nullptr,
                  uint32_t* amax = nullptr);
// behind an owned-sums launch, on the same stream (e3_msg_owned.hip): the rows of the chunk-boundary nodes from their partial
// sums (part / part_node, nslots = 2 x chunks; their max |x| joins `amax`), and zeros for the nodes without an incoming edge
int msg_owned_finish(const float* part, const int* part_node, int64_t nslots, const int32_t* dst, int64_t E, int64_t N, int D,
                     float* out, int64_t ldo, uint32_t* amax, hipStream_t s);
int scale_finalize(float* out4, int target_log2, hipStream_t s);  // {s, 1/s} from the float bits at out4[2] (e3_scale.hip)
int msg_ws_chunk_edges(int chunk_edges);                    // edges per chunk the launch uses
int64_t msg_ws_owned_chunks(int64_t E, int chunk_edges);     // chunk slots of an owned-sums launch (8 x chunks per eighth)
}  // namespace e3
