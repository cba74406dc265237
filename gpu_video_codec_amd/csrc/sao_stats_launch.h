/* sao_stats_launch.h -- PRIVATE to the library: the launches of sao_stats.hip as sao_stats_host.cpp calls them */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sao_stats.h"

/* every row of both planes starts at a multiple of four samples: the kernel that moves four samples per load runs */
bool dbk_sao_stats_vec(const DbkSaoStatsArgs &a, int sample_bytes);
hipError_t dbk_launch_sao_stats(const DbkSaoStatsArgs &a, int sample_bytes, hipStream_t stream);
hipError_t dbk_launch_sao_pick(const DbkSaoPickArgs &a, hipStream_t stream);
