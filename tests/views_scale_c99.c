/* Compiled as C99 by tests/test_views_scale_host.py: umetrack_hip_views_scale.h must be usable from C. */
#include "umetrack_hip_views_scale.h"

int views_scale_c99_probe(void) {
  int (*fit)(ut_handle, const float*, int, const double*, const float*, const int32_t*, int, const double*, int, int, const float*,
             const float*, int, const float*, int, const float*, int, const int64_t*, float, int, int, float, int, float*, int,
             float*, int, float*, float*, float*, float*, void*) = ut_fit_pose_views_scale;
  return (fit != 0) + UT_LOSS_SQUARED + UT_LOSS_HUBER + UT_LOSS_GEMAN_MCCLURE + UT_SCALE_FREE + UT_SCALE_FIXED + UT_FITS_AT_BOUND +
         UT_TRI_MAX_VIEWS + (UT_SCALE_MIN < UT_SCALE_MAX);
}
