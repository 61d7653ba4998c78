/* Compiled as C99 by tests/test_smooth_host.py: umetrack_hip_smooth.h must be usable from C. */
#include "umetrack_hip_smooth.h"

int smooth_c99_probe(void) {
  int (*smooth)(ut_handle, const float*, int, const float*, int, const float*, const float*, const float*, const int32_t*, const float*,
                const float*, int, float, int, int, float*, float*, int, float*, int, float*, float*, void*) = ut_smooth_pose_sequence;
  return (smooth != 0) + UT_SMOOTH_OK + UT_SMOOTH_GAP + UT_SMOOTH_SINGULAR + UT_SMOOTH_REFUSED + UT_SMOOTH_WORK + (UT_COV_MIN_PIVOT > 0.0f) +
         UT_FIT_REFUSED;
}
