/* Compiled by tests/test_mesh_host.py with a plain C compiler in C99 mode: the mesh entries are part of the boundary header,
 * with the declared types. */
#include <stdint.h>

#include "umetrack_hip.h"

typedef int (*type_ut_mesh_create)(const float*, int, const int32_t*, int, const float*, int, ut_mesh**);
typedef int (*type_ut_mesh_destroy)(ut_mesh*);
typedef int (*type_ut_mesh_counts)(const ut_mesh*, int*, int*);
typedef int (*type_ut_skin_mesh)(ut_handle, const ut_mesh*, const float*, int, const float*, int, const float*, int,
                                 const int64_t*, float, int, float*, float*, void*);

type_ut_mesh_create mesh_create_entry(void) { return ut_mesh_create; }
type_ut_mesh_destroy mesh_destroy_entry(void) { return ut_mesh_destroy; }
type_ut_mesh_counts mesh_counts_entry(void) { return ut_mesh_counts; }
type_ut_skin_mesh skin_mesh_entry(void) { return ut_skin_mesh; }

typedef char cap_is_at_least_4096[UT_MESH_MAX_VERTICES >= 4096 ? 1 : -1];
typedef char four_influences[UT_MESH_MAX_INFLUENCES == 4 ? 1 : -1];
