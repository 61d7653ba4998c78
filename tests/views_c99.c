/* Compiled as C99 by tests/test_views_host.py: umetrack_hip_views.h must be usable from C. */
#include "umetrack_hip_views.h"

int views_c99_probe(void) {
  int (*fit)(ut_handle, const float*, int, const double*, const float*, const int32_t*, int, const double*, int, int, const float*,
             const float*, int, const float*, int, const int64_t*, float, int, int, float*, int, float*, int, float*, float*,
             void*) = ut_fit_pose_views;
  return (fit != 0) + UT_FIT_CONVERGED + UT_FIT_AT_MAX_ITERS + UT_FIT_REFUSED + UT_TRI_MAX_VIEWS + UT_CAMERA_PINHOLE;
}
