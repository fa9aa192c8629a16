// mesh_compact.h -- the ordered compaction of mesh_kernels.hip, for the other mesh sources of the library (internal: no entry point).
#pragma once
#include "gp_common.h"

// rank[e] = the number of e' < e with keep[e'] != 0, for every e < n; *total = the number of all of them (on the device).  Per tile of
// GP_MESH_TILE elements a sum, ONE workgroup scans the tiles in place, ballot ranks inside the tile: no atomics, one order.
// tile_sums: [ceil(n / GP_MESH_TILE)] words of scratch.  n = 0 is accepted (the total is still written).  Returns != 0 (and
// gp_last_error()) where a launch fails.
int ms_compact(const uint8_t* keep, uint32_t n, uint32_t* tile_sums, uint32_t* rank, int32_t* total, hipStream_t st);
