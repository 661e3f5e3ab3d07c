// Launch of the one-wave-per-tile message kernel (e3_msg_fused_kernel.h; instantiated per storage type by
// e3_msg_fused_f32.hip and e3_msg_fused_bf16.hip): the kernel of every shape the weights-stationary kernel (e3_msg_ws.hip) does not take,
// and of tiles_per_block < 0.
#include "e3_msg_plan.h"

#include <algorithm>

namespace e3 {

static const void* fused_kernel(const MsgShape& k, PbcMode mode, int io) {
  static const MsgFusedKernels* const table[2] = {&msg_fused_kernels_f32(), &msg_fused_kernels_bf16()};
  return table[io]->k[mode][k.index];
}

// dynamic LDS of a workgroup: the tables, the four waves' images and their edge-id buffers
static size_t fused_lds_bytes(const MsgShape& k) { return (size_t)(k.lds_tab + 4 * k.lds_wave) * 4 + 4 * 256; }

int msg_fused_setup(const MsgShape& k, PbcMode mode, int io, int dev, int* workgroups) {
  struct Grids { int wg[kMsgShapes][3][2]; };
  static std::mutex mu;
  static std::vector<Grids> grids;  // per device; 0 = not set up
  if (dev < 0) return E3_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)grids.size() <= dev) grids.resize(dev + 1, Grids{});
  int& wg = grids[dev].wg[k.index][mode][io];
  if (!wg) {
    // The grid fills the chip exactly once: what the registers the compiler ended up with and the LDS image allow per CU
    // (2 workgroups for H = 32, l_max = 2; the small instantiations fit 3-4), not a number assumed at compile time.
    const void* kern = fused_kernel(k, mode, io);
    const size_t lds = fused_lds_bytes(k);
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    // the occupancy query comes after the limit is raised: it answers for the limit in force
    if (!kern || ensure_dyn_lds(kern, lds) != E3_OK ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu < 1)
      return E3_ERR_HIP;
    wg = cus * (per_cu < 4 ? per_cu : 4);
  }
  if (workgroups) *workgroups = wg;
  return E3_OK;
}

int msg_fused_launch(const e3_msg_plan& P, const MsgOperands& a, const MsgPbc& pbc) {
  const MsgShape& k = *P.k;
  const int io = a.dtype == E3_BF16 ? 1 : 0;
  const int tiles_per_block = a.tiles_per_block < 0 ? -a.tiles_per_block : a.tiles_per_block;
  int nwg = 0;  // 4 waves per workgroup, every CU filled once
  const int st = msg_fused_setup(k, pbc.mode, io, P.device, &nwg);
  if (st != E3_OK) return st;
  const int64_t ntiles = (a.E + 15) / 16;
  nwg = (int)std::min<int64_t>(nwg, (ntiles + 3) / 4);
  nwg = std::max(8, (nwg + 7) / 8 * 8);
  int blk = tiles_per_block > 0 ? tiles_per_block : 4;  // default: 64 edges (2-3 dst nodes) per wave block
  if (blk > (1 << 16)) blk = 1 << 16;
  // the kernel's parameter list (MsgFusedKernarg, e3_msg_fused_kernel.h): the box or the cell of the mode comes last
  void* args[] = {(void*)&a.h, (void*)&a.ld_h, (void*)&a.pos4, (void*)&a.src, (void*)&a.dst, (void*)&a.E, (void*)&a.packed,
                  (void*)&a.premix, (void*)&a.in_scale, (void*)&a.out, (void*)&a.ld_out, &blk, (void*)pbc.kernel_arg()};
  if (hipLaunchKernel(fused_kernel(k, pbc.mode, io), dim3(nwg), dim3(256), args, fused_lds_bytes(k), a.stream) != hipSuccess)
    return E3_ERR_HIP;
  return E3_OK;
}

}  // namespace e3
