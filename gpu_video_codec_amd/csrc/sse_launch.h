/* sse_launch.h -- PRIVATE to the library: the launches of sse.hip as sse_host.cpp calls them */
#pragma once
#include <hip/hip_runtime_api.h>

#include "sse.h"

/* how the rows of both planes are fetched: sse::kWide where every row of both starts at a multiple of 16 bytes, sse::kQuad at a
 * multiple of four samples, else sse::kScalar */
int dbk_sse_mode(const DbkSseArgs &a, int sample_bytes);
hipError_t dbk_launch_sse(const DbkSseArgs &a, int sample_bytes, hipStream_t stream);
hipError_t dbk_launch_sse_sp(const DbkSseArgs &a, int sample_bytes, hipStream_t stream); /* a plane of pairs: a.sse_odd set */
hipError_t dbk_launch_sse_totals(const DbkSseTotalsArgs &a, hipStream_t stream);
