/* sao_decide_launch.h -- PRIVATE to the library: the launches of sao_decide.hip as sao_decide_host.cpp calls them */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sao_decide.h"

/* the NEW launch, then the MERGE launch (none for a grid of one CTB), on one stream */
hipError_t dbk_launch_sao_decide(const DbkSaoDecideArgs &a, hipStream_t stream);
/* the MERGE launch alone, for whoever wrote the NEW triples and records with a launch of its own (sao_pick_os.hip) */
hipError_t dbk_launch_sao_decide_merge(const DbkSaoDecideArgs &a, hipStream_t stream);
