/* sao_slice_launch.h -- PRIVATE to the library: the launches of sao_slice.hip as sao_decide_host.cpp calls them */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sao_decide_launch.h"
#include "sao_slice.h"

/* the NEW launch under the caller's flag bytes, then sao_decide.hip's MERGE launch (none for a grid of one CTB), on one stream */
hipError_t dbk_launch_sao_decide_sf(const DbkSaoSliceArgs &s, hipStream_t stream);
/* the choice: NEW into the workspace's three states, the walk of one workgroup per frame, the final copy; n_slices <= saoslice::kMaxSlices */
hipError_t dbk_launch_sao_slice_flags(const DbkSaoSliceArgs &s, hipStream_t stream);
