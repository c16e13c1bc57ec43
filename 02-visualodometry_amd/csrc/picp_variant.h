// picp_variant.h -- which per-item math a launch runs: the variants' numbers (template arguments
// of the kernels) and the host's launch-time choice among them.  Host code; nothing here is HIP.
#pragma once
#include <stdlib.h>

// Per-item math variant, fixed at launch (picp_variant): any K with the kernel weight chosen at
// run time; the reference's pinhole K with outliers rejected (keep_outliers = false, as
// icp_test runs it: every used item has weight exactly 1, so the weighted Jacobian IS the
// Jacobian and no weight is formed); pinhole K with outliers kept (robust weight per item).
#define PICP_V_GENERAL 0
#define PICP_V_PINHOLE 1
#define PICP_V_PINHOLE_KEEP 2

namespace picp {

inline bool is_pinhole(const float K[9]) {  // column-major K
  return K[1] == 0.0f && K[2] == 0.0f && K[3] == 0.0f && K[5] == 0.0f && K[8] == 1.0f;
}

}  // namespace picp

// launch-time camera path: pinhole unless K is general or PICP_FORCE_GENERAL_K=1 (A/B checks)
inline bool picp_use_pinhole(const float K[9]) {
  static const bool force_general = [] {
    const char* e = getenv("PICP_FORCE_GENERAL_K");
    return e && atoi(e) != 0;
  }();
  return !force_general && picp::is_pinhole(K);
}

// launch-time per-item variant (PICP_V_*): the camera path, and for the pinhole path whether
// outliers are kept (a compile-time weight)
inline int picp_variant(const float K[9], int keep_outliers) {
  if (!picp_use_pinhole(K)) return PICP_V_GENERAL;
  return keep_outliers ? PICP_V_PINHOLE_KEEP : PICP_V_PINHOLE;
}
