// What the host files of the SEGNN message function (e3_msg_*, include/e3gnn.h) share:
//   e3_msg_pack.hip     plans, weight packing                 e3_msg_premix.hip   the per-node launches
//   e3_msg_forward.hip  the six e3_msg_forward* entries: checks, owned-sums orchestration, choice of the edge kernel
//   e3_msg_ws.hip       the weights-stationary edge kernel (H = 32) and its launch
//   e3_msg_fused.hip    the launch of the one-wave-per-tile edge kernel (kernel: e3_msg_fused_kernel.h, instantiated per
//                       storage type by e3_msg_fused_f32.hip -- with the packing kernels -- and e3_msg_fused_bf16.hip)
//   e3_msg_owned.hip    the two small kernels behind an owned-sums launch
// Private header; the device pieces the kernels share are in e3_msg_common.h.
#pragma once
#include "e3_common.h"

namespace e3 {

// The (l_max, H = 16 tt) pairs the message kernels are instantiated for: X(index, l_max, tt).  Every kernel table is written
// with this list and indexed by MsgShape::index.
#define E3_MSG_SHAPES(X) X(0, 2, 2) X(1, 1, 2) X(2, 2, 1) X(3, 1, 1) X(4, 2, 4) X(5, 1, 4)
constexpr int kMsgShapes = 6;

// geometry of one pair (MsgGeom<l_max, tt>, e3_msg_common.h) as the host needs it
struct MsgShape {
  int index, lmax, tt;
  bool bf16;  // bf16 storage is instantiated: the [0e] region of a staged row must be at least 4 units of 16 bytes (H >= 32)
  int64_t total_floats;
  int UD, D, lds_tab, lds_wave, nblk, NS, WD, o_norm1, o_norm2, o_wd, o_w;
};

struct MsgPackDesc {  // one weight block
  int role;           // 0: TP #1 src rows, 1: TP #2, 2: TP #1 dst rows (pre-mix)
  int mat;            // output degree l3 = class matrix index
  int rowbase;        // row of channel 0 of this K step in the class matrix
  int nvalid;         // channels of this K step that exist (<= 32)
  int M, colbase;     // matrix width, first output channel of the tile
  int blk;            // block index inside the role
};
struct MsgPackArgs {
  const void* w1[3];
  const void* w2[3];
  const void* n1[3];
  const void* n2[3];
  int64_t nw1[3], nw2[3];  // elements per class matrix
  int rowd[3];             // row of the distance channel in class l's matrix (path (0, l, l)), TP #1
  int M0, H, LMAX, TT, NS, WD, o_norm1, o_norm2, o_wd, o_w, nblk;
};

// Periodicity of one call, built once by the C entry: mode = the kernel instantiation (an all-zero box of e3_msg_forward_pbc
// is kBox, not kOpen); `box` is what make_box derived (zeros for kOpen: the open kernels carry an unread PbcBox), `cell` what
// make_cell derived (kCell only).
struct MsgPbc {
  PbcMode mode = kOpen;
  PbcBox box = {};
  PbcCell cell = {};
  const void* kernel_arg() const { return mode == kCell ? (const void*)&cell : (const void*)&box; }
};

// The operands of e3_msg_forward* (include/e3gnn.h) as the entries received them
struct MsgOperands {
  const void* h; int64_t ld_h; int64_t N;
  const float* pos4; const int32_t *src, *dst; int64_t E;
  const void* packed; const float* in_scale; const float* premix;
  float* out; int64_t ld_out;
  int dtype, accumulate, tiles_per_block;
  hipStream_t stream;
};
// ... and what the owned-sums entries (e3_msg_forward_owned*) take on top
struct MsgOwned {
  void* workspace; int64_t workspace_bytes;
  float* out_scale4; int target_log2;
};
// Owned sums inside the weights-stationary launch, for a launch that does not accumulate.  `out` needs no zero-fill: the
// kernel stores the rows whose run lies inside one chunk itself and joins their max |x| (finite values) into the max-bits
// word `amax`; the first and the last flushed node of chunk c leave their partial sums in part[2 c + {0, 1}][D] and their ids
// in part_node[2 c + {0, 1}] (preset to -1 by the caller; msg_ws_owned_chunks chunks, in edge order), for the boundary merge
// behind the launch.
struct MsgWsOwned {
  float* part; int* part_node; uint32_t* amax;
};

}  // namespace e3

struct e3_msg_plan {
  int lmax, H;
  const e3::MsgShape* k;
  std::vector<e3::MsgPackDesc> desc;
  int rowd[3];
  int K1[3], K2[3], M[3];
  e3::MsgPackDesc* d_desc = nullptr;
  int device = -1;
  std::mutex mu;
};

namespace e3 {

// e3_msg_pack.hip.  First use of a plan on the device (pack_weights, premix or forward): the pack descriptors are uploaded
// and the open and box instantiations of the one-wave-per-tile kernel are set up (msg_fused_setup); the plan then belongs to
// that device
int msg_ensure_device(e3_msg_plan* P);

// e3_msg_fused_f32.hip: the packing kernels on stream s (the header of `packed` zeroed first)
int msg_pack_launch(const MsgPackArgs& a, const MsgPackDesc* d_desc, int ndesc, int dtype, void* packed, hipStream_t s);

// ---- e3_msg_fused.hip: the one-wave-per-tile kernel ----
// The kernels of one storage type, [PbcMode][shape index] (nullptr: not instantiated); each table stands in the file that
// instantiates its kernels (e3_msg_fused_f32.hip, e3_msg_fused_bf16.hip)
struct MsgFusedKernels { const void* k[3][kMsgShapes]; };
const MsgFusedKernels& msg_fused_kernels_f32();
const MsgFusedKernels& msg_fused_kernels_bf16();
// Once per device, shape, mode and storage type: the LDS image admitted and the workgroups of a full launch (`workgroups`,
// optional) from the occupancy query.  msg_ensure_device calls it for the open and box instantiations; the cell
// instantiations are set up by their first launch (a plan that only ever sees open or orthorhombic graphs never touches them).
int msg_fused_setup(const MsgShape& k, PbcMode mode, int io, int device, int* workgroups);
// Operands after the checks of e3_msg_forward, E > 0, `out` zeroed or holding the sums to continue (atomics).
// |tiles_per_block| = tiles per wave block (0 = default 4).
int msg_fused_launch(const e3_msg_plan& P, const MsgOperands& a, const MsgPbc& pbc);

// ---- e3_msg_ws.hip: the weights-stationary kernel ----
// l_max = 1 does not take it: correct, but 10.0 vs 6.4 ms per launch pair against the one-wave-per-tile kernel (the phase
// structure does not pay for so little work per edge)
bool msg_ws_supported(int lmax, int hidden, int dtype);
// floats per node of the pre-split rows the fp32 kernel gathers (MsgSplit, e3_msg_common.h); 0: the shape never takes this kernel
int msg_ws_split_floats(int lmax, int hidden);
// edges per chunk of the workgroups' round-robin: 16 * tiles_per_block (0 = default 256; clamped to 2^24)
int msg_ws_chunk_edges(int tiles_per_block);
// chunk slots of an owned-sums launch (8 x chunks per eighth)
int64_t msg_ws_owned_chunks(int64_t E, int tiles_per_block);
// Operands after the checks of e3_msg_forward, E > 0.  `a.premix` = what e3_msg_premix wrote: N table rows, the N pre-split
// rows, then the N per-node row maxima of h * in_scale (msg_premix_layout).  owned == nullptr: the sums arrive by atomics in
// `out`, which is zeroed or holds the sums to continue (the accumulating launches: sharded and continued sums).
// E3_ERR_UNSUPPORTED: nothing launched, the caller takes the other kernel.
int msg_ws_launch(const e3_msg_plan& P, const MsgOperands& a, const MsgPbc& pbc, const MsgWsOwned* owned);

// ---- e3_msg_owned.hip ----
// behind an owned-sums launch, on the same stream: the rows of the chunk-boundary nodes from their partial sums (part /
// part_node, nslots = 2 x chunks; their max |x| joins `amax`), and zeros for the nodes without an incoming edge
int msg_owned_finish(const float* part, const int* part_node, int64_t nslots, const int32_t* dst, int64_t E, int64_t N, int D,
                     float* out, int64_t ldo, uint32_t* amax, hipStream_t s);
int scale_finalize(float* out4, int target_log2, hipStream_t s);  // {s, 1/s} from the float bits at out4[2] (e3_scale.hip)

}  // namespace e3
