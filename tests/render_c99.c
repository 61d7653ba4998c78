/* Compiled by tests/test_render_host.py with a plain C compiler in C99 mode: the projection and render entries are part of
 * the boundary header, with the declared types. */
#include <stdint.h>

#include "umetrack_hip.h"

typedef int (*type_ut_project_points)(ut_handle, const float*, int, int, const int32_t*, int, const double*, int, int, int, int,
                                      int, double*, double*, uint8_t*, void*);
typedef int (*type_ut_render_mesh)(ut_handle, const ut_mesh*, const float*, const double*, int, const int64_t*, int, int,
                                   float*, int32_t*, uint8_t*, void*);

type_ut_project_points project_points_entry(void) { return ut_project_points; }
type_ut_render_mesh render_mesh_entry(void) { return ut_render_mesh; }

typedef char the_hand_mesh_fits[UT_RENDER_MAX_VERTICES >= 788 && UT_RENDER_MAX_VERTICES <= UT_MESH_MAX_VERTICES ? 1 : -1];
typedef char camera_kinds[UT_CAMERA_FISHEYE62 == 0 && UT_CAMERA_PINHOLE == 1 ? 1 : -1];
