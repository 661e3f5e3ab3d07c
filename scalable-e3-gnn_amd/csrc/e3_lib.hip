// The library's runtime: the HIP error record, the dynamic-LDS limit of a kernel, and the ABI entries that describe the
// library itself (version, status strings, last HIP error).  No kernels.
#include "e3_common.h"

#include <map>
#include <mutex>
#include <utility>

namespace e3 {

static thread_local std::string g_hip_err;
void set_hip_error(hipError_t e, const char* what) {
  g_hip_err = std::string(hipGetErrorName(e)) + ": " + hipGetErrorString(e) + " in " + what;
}

int ensure_dyn_lds(const void* fn, size_t bytes) {
  if (bytes <= 64 * 1024) return E3_OK;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> have;
  int dev = 0;
  E3_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  size_t& cur = have[std::make_pair(fn, dev)];
  if (bytes > cur) {
    E3_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    cur = bytes;
  }
  return E3_OK;
}

}  // namespace e3

using namespace e3;

extern "C" {

int e3_abi_version(void) { return E3GNN_ABI_VERSION; }

const char* e3_status_string(int s) {
  switch (s) {
    case E3_OK: return "ok";
    case E3_ERR_INVALID_ARG: return "invalid argument";
    case E3_ERR_BAD_IRREPS: return "bad irreps (need l in {0,1}, lmax == 1, p in {+1,-1}, mul >= 0)";
    case E3_ERR_MISSING_WEIGHT: return "an output class has columns but no weight matrix";
    case E3_ERR_UNSUPPORTED: return "unsupported shape/dtype for the requested kernel";
    case E3_ERR_HIP: return "HIP runtime error";
    case E3_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown status";
  }
}

const char* e3_last_hip_error(void) { return g_hip_err.c_str(); }

}  // extern "C"
