/* Compiled by tests/test_triangulate_host.py with a plain C compiler in C99 mode: ut_triangulate_points is declared by the
 * extension header umetrack_hip_triangulate.h on its own, with these types, status bits and constants. */
#include <stdint.h>

#include "umetrack_hip_triangulate.h"

typedef int (*type_ut_triangulate_points)(ut_handle, const double*, const float*, const int32_t*, int, const double*, int, int, int,
                                          int, int, double*, float*, int, float*, float*, void*);

type_ut_triangulate_points triangulate_entry(void) { return ut_triangulate_points; }

typedef char status_bits[(UT_TRI_CONVERGED == 1 && UT_TRI_AT_MAX_ITERS == 2 && UT_TRI_REFUSED == 4 && UT_TRI_DEGENERATE == 8) ? 1 : -1];
typedef char view_cap[(UT_TRI_MAX_VIEWS == 8) ? 1 : -1];
static const double thresholds[] = {UT_TRI_PIVOT_FRACTION, UT_TRI_LAMBDA_START, UT_TRI_LAMBDA_MIN, UT_TRI_LAMBDA_CONVERGED_MAX,
                                    UT_TRI_STEP_TOL, UT_TRI_FLAT_TOL_PX, UT_TRI_NEAR_Z};
const double* triangulate_thresholds(void) { return thresholds; }
