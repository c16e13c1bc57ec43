// picp_runtime.cpp -- what every part of the host runtime behind the C-ABI (include/picp_c.h)
// shares: the thread's last error, the ABI version and parameter defaults, the device count and
// selection, and the helpers of picp_host.h.  The subsystems are in picp_batch.cpp (batch solver),
// picp_batch_classify.cpp, picp_handle.cpp (single-problem handle), picp_frontend.cpp,
// picp_refine_runtime.cpp, picp_vo_runtime.cpp and picp_comm.cpp.  No torch, no host fallback:
// every compute entry point runs the HIP kernels or fails with PICP_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "picp_c.h"
#include "picp_host.h"

// ------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------
static thread_local std::string g_err;

int picp_set_err(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define set_err picp_set_err

extern "C" const char* picp_last_error(void) { return g_err.c_str(); }
extern "C" int picp_abi_version(void) { return PICP_ABI_VERSION; }

extern "C" void picp_params_default(picp_params* p) {
  if (!p) return;
  p->threshold = 1000.0f;  // src/picp_solver.cpp:14
  p->damping = 1.0f;       // src/picp_solver.cpp:11
  p->min_inliers = 0;      // src/picp_solver.cpp:12
  p->keep_outliers = 0;    // exec/icp_test.cpp:95
  p->max_rounds = 50;      // exec/icp_test.cpp:88
  p->conv_eps = 1e-5f;     // exec/icp_test.cpp:91
}

extern "C" int picp_device_count(int* n) {
  CHECK_ARG(n, "picp_device_count: null output");
  int c = 0;
  HIP_TRY(hipGetDeviceCount(&c));
  *n = c;
  return PICP_OK;
}

int select_device(const char* what, int device) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_err(PICP_ERR_ARG, "%s: no such HIP device", what);
  HIP_TRY(hipSetDevice(device));
  return PICP_OK;
}

// ------------------------------------------------------------------------------------
// state helpers (the pose conversions: picp_pose.h)
// ------------------------------------------------------------------------------------
void state_to_stats(const PicpState& s, picp_stats& st) {
  st.chi_in = s.chi_in;
  st.chi_out = s.chi_out;
  st.n_in = s.n_in;
  st.ok = s.ok;
  st.rounds = s.rounds;
  st.converged = s.converged;
  st.n_projected = s.n_proj;
  st.reserved = 0;
}

int grow(void** ptr, int64_t* cap, int64_t need, size_t elem) {
  if (need <= *cap) return PICP_OK;
  if (*ptr) hipFree(*ptr);
  *ptr = nullptr;
  const int64_t c = std::max<int64_t>(need, 256);
  hipError_t e = hipMalloc(ptr, (size_t)c * elem);
  if (e != hipSuccess) { *cap = 0; return set_err(PICP_ERR_NOMEM, "hipMalloc(%zu): %s", (size_t)c * elem, hipGetErrorString(e)); }
  *cap = c;
  return PICP_OK;
}
