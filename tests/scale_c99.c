/* Compiled as C99 by tests/test_scale_host.py: umetrack_hip_scale.h must be usable from C. */
#include "umetrack_hip_scale.h"

int scale_c99_probe(void) {
  int (*fit)(ut_handle, const float*, int, const float*, int, const float*, const float*, const float*, int, const float*, int,
             const float*, int, const int64_t*, float, int, int, float*, int, float*, int, float*, float*, void*) = ut_fit_pose_scale;
  int (*pool)(ut_handle, const float*, const float*, int, int, float*, float*, void*) = ut_pool_scale;
  float lo = UT_SCALE_MIN, hi = UT_SCALE_MAX, lambda = UT_SCALE_INFO_LAMBDA;
  return (fit != 0) + (pool != 0) + (lo < hi) + (lambda > 0.0f) + UT_SCALE_FREE + UT_SCALE_FIXED + UT_FITS_CONVERGED +
         UT_FITS_AT_MAX_ITERS + UT_FITS_REFUSED + UT_FITS_AT_BOUND;
}
