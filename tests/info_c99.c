/* Compiled as C99 by tests/test_info_host.py: umetrack_hip_info.h must be usable from C. */
#include "umetrack_hip_info.h"

int info_c99_probe(void) {
  int (*tri)(ut_handle, const double*, const float*, const int32_t*, int, const double*, int, int, int, int, int, double*, float*,
             int, float*, float*, float*, void*) = ut_triangulate_points_info;
  int (*fit)(ut_handle, const float*, int, const float*, int, const float*, const float*, const float*, int, const float*, int,
             const int64_t*, float, int, int, float*, int, float*, int, float*, void*) = ut_fit_pose_info;
  float factor[UT_INFO_FACTOR_FLOATS] = {0};
  return (tri != 0) + (fit != 0) + (int)factor[5] + UT_FIT_CONVERGED + UT_FIT_AT_MAX_ITERS + UT_FIT_REFUSED + UT_TRI_CONVERGED;
}
