/* Compiled as C99 by tests/test_start_host.py: umetrack_hip_start.h must be usable from C. */
#include "umetrack_hip_start.h"

int start_c99_probe(void) {
  int (*start)(ut_handle, const float*, int, const double*, const float*, const int32_t*, int, const double*, int, int, const float*,
               const float*, int, const double*, int, const int64_t*, float, int, int, float*, int, float*, int, float*, void*) =
      ut_start_pose_views;
  int (*select)(const float*, int, const float*, int, const float*, int, int, float*, int, float*, int, float*, int32_t*, void*) =
      ut_select_pose;
  return (start != 0) + (select != 0) + UT_START_MAX_SEEDS + UT_FIT_REFUSED + UT_TRI_MAX_VIEWS;
}
