/* Compiled by tests/test_fit_host.py with a plain C compiler in C99 mode: ut_fit_pose is declared by the extension header
 * umetrack_hip_fit.h, with these types and status bits. */
#include <stdint.h>

#include "umetrack_hip_fit.h"

typedef int (*type_ut_fit_pose)(ut_handle, const float*, int, const float*, int, const float*, const float*, const float*, int,
                                const float*, int, const int64_t*, float, int, int, float*, int, float*, int, float*, void*);

type_ut_fit_pose fit_pose_entry(void) { return ut_fit_pose; }

typedef char status_bits[(UT_FIT_CONVERGED == 1 && UT_FIT_AT_MAX_ITERS == 2 && UT_FIT_REFUSED == 4) ? 1 : -1];
