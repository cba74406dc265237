/* entry_sim.h -- what a case of tests/entry_sim sets for the stubs (stubs.cpp) and what they record for it. */
#pragma once
#include <string>

struct SimCtl {
    bool set_device_fails = false;  /* hipSetDevice, i.e. dbkh::bind, fails */
    int fail_at = 0;                /* the k-th launch of the case returns an error (0 = none) */
    /* the answers of the *_supports predicates: bit i for plane i asked as a luma plane, bit 4 + i asked as a chroma
     * plane; the plane is told by its src address (sim_plane_base) */
    unsigned packed_mask = 0, fused_mask = 0, sp_mask = 0;
    int n_launch = 0, n_dev = 0, n_ev = 0, n_stream = 0;
    std::string trace;              /* one line per launch, event call and stream call */
};
extern SimCtl g_sim;

/* the caller's plane i starts at this address; anything else an entry hands to a kernel is scratch the stubs allocated */
inline unsigned long long sim_plane_base(int i) { return 0x10000000ull * (unsigned long long)(i + 1); }
/* a pointer as the trace names it: 0, dev<k>+<offset> for memory of the k-th hipMalloc of the case, else its value */
std::string sim_ptr(const void *p);
/* dev<k> of a pointer hipMalloc returned, "-" for none */
std::string sim_dev_name(const void *p);
std::string sim_event_name(const void *e);
/* forget the allocations' names (a new context follows) */
void sim_new_case();
