// The one-wave-per-tile message kernel (e3_msg_fused_kernel.h), bf16-storage instantiations of all three periodicity modes
// (the fp32 ones: e3_msg_fused_f32.hip).
#include "e3_msg_plan.h"
#include "cg_tables.h"

#include <cstddef>
#include <type_traits>
#include <utility>

namespace e3 {
#include "e3_tp_mfma_core.h"
#include "e3_msg_common.h"
#include "e3_msg_fused_kernel.h"

const MsgFusedKernels& msg_fused_kernels_bf16() {
  static const MsgFusedKernels k = msg_fused_kernels<true>();
  return k;
}
}  // namespace e3
