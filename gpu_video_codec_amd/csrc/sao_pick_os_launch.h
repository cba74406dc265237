/* sao_pick_os_launch.h -- PRIVATE to the library: the launches of sao_pick_os.hip as sao_stats_host.cpp and sao_decide_host.cpp call them */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sao_decide_launch.h"
#include "sao_pick_os.h"

hipError_t dbk_launch_sao_pick_os(const DbkSaoPickOsArgs &a, hipStream_t stream);
/* the NEW launch with the scales, then sao_decide.hip's MERGE launch (none for a grid of one CTB), on one stream */
hipError_t dbk_launch_sao_decide_os(const DbkSaoDecideOsArgs &a, hipStream_t stream);
