/* sao_stats_sp_launch.h -- PRIVATE to the library: the launch of sao_stats_sp.hip as sao_stats_host.cpp calls it */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sao_stats_sp.h"

/* every row of both planes starts at a multiple of four pairs: the kernel that moves four pairs per load runs */
bool dbk_sao_stats_sp_vec(const DbkSaoStatsSpArgs &a, int sample_bytes);
/* dynamic LDS of the launch: 2 x max(16, CTBs per region) x 53 x 8 bytes */
size_t dbk_sao_stats_sp_lds(int ctb_log2);
hipError_t dbk_launch_sao_stats_sp(const DbkSaoStatsSpArgs &a, int sample_bytes, hipStream_t stream);
