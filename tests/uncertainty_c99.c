/* Compiled as C99 by tests/test_uncertainty_host.py: umetrack_hip_uncertainty.h must be usable from C. */
#include "umetrack_hip_uncertainty.h"

int uncertainty_c99_probe(void) {
  int (*cov)(ut_handle, const float*, int, const double*, const float*, const int32_t*, int, const double*, int, int, const float*,
             const float*, int, const float*, int, const int64_t*, float, int, float, int, float*, float*, float*, float*, float*,
             void*) = ut_pose_information_views;
  return (cov != 0) + UT_COV_OK + UT_COV_SINGULAR + UT_COV_REFUSED + (UT_COV_MIN_PIVOT > 0.0f) + UT_LOSS_HUBER + UT_FIT_REFUSED;
}
