// enc_sums_sim.cpp -- the model waves' sums of a group (TEST TOOLING, not part of librcx.so).
//
// Compiles rcx_pre4 / rcx_pre4_sel4 / rcx_sel4 of cpprcoder_amd/csrc/rcx_lane.hpp for the host -- the chains of 24-bit
// multiply-adds as the kernels form them, with the host's rcx_mul24 masking its factors to 24 bits as v_mad_u32_u24 does
// -- and runs them over arrays of groups for tests/test_enc_sums_cpu.py.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../cpprcoder_amd/csrc/rcx_lane.hpp"

uint64_t rcx_sim_counters[4] = {0, 0, 0, 0};

// groups: n x 4 counts; for every group and every p in 0..3: sums[4 i + p] = rcx_pre4, counts[4 i + p] = rcx_sel4, and the
// pair from rcx_pre4_sel4 in both_sums / both_counts
extern "C" void sim_group_sums(const uint32_t* groups, uint64_t n, uint32_t* sums, uint32_t* counts, uint32_t* both_sums,
                               uint32_t* both_counts)
{
    for (uint64_t i = 0; i < n; ++i) {
        U4 g;
        g.x = groups[4 * i], g.y = groups[4 * i + 1], g.z = groups[4 * i + 2], g.w = groups[4 * i + 3];
        for (u32 p = 0; p < 4; ++p) {
            sums[4 * i + p] = rcx_pre4(g, p);
            counts[4 * i + p] = rcx_sel4(g, p);
            u32 f = 0;
            both_sums[4 * i + p] = rcx_pre4_sel4(g, p, f);
            both_counts[4 * i + p] = f;
        }
    }
}
