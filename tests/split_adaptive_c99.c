/* Compiled by tests/test_split_adaptive_host.py with a plain C compiler in C99 mode: the adaptive split-scale mode and its
 * counter entry are part of the boundary header, with the declared types. */
#include <stdint.h>

#include "umetrack_hip.h"

typedef int (*type_ut_get_split_adaptations)(ut_handle, uint32_t*, int, void*);

int split_adaptive_mode(void) { return UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE; }

type_ut_get_split_adaptations split_adaptations_entry(void) { return ut_get_split_adaptations; }

typedef char adaptive_is_two[UT_SPLIT_SCALE_CALIBRATED_ADAPTIVE == 2 ? 1 : -1];
typedef char modes_distinct[UT_SPLIT_SCALE_CALIBRATED != UT_SPLIT_SCALE_DYNAMIC ? 1 : -1];
