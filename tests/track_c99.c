/* Compiled as C99 by tests/test_track_host.py: umetrack_hip_track.h must be usable from C. */
#include "umetrack_hip_track.h"

int track_c99_probe(void) {
  int (*track)(ut_handle, const float*, int, const double*, const float*, const int32_t*, int, const double*, int, int, const float*,
               const float*, int, const float*, int, const float*, int, const float*, int, const float*, const int32_t*, double, double,
               const int32_t*, const int64_t*, float, int, int, float, int, int, float*, int, float*, int, float*, int32_t*, void*) =
      ut_track_pose_views;
  return (track != 0) + UT_TRACK_WARM + UT_TRACK_COLD + UT_TRACK_NONE + UT_START_MAX_SEEDS + UT_FIT_REFUSED;
}
