// Spec: e3_common.h.  rocprim's scan is over a hundred kernels per instantiation, so there is exactly this one.
#include "e3_common.h"

#include <hipcub/hipcub.hpp>

namespace e3 {

size_t scan_temp_bytes(int64_t n) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  return t;
}

hipError_t exclusive_sum(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n, s);
}

}  // namespace e3
