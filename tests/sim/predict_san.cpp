// predict_san.cpp -- predict_sim.cpp's functions in a program of its own, to be built with -fsanitize=address,undefined
// (tests/test_predict_cpu.py does): for every width and both predictors, units of all-ones, zeros and random bytes go
// forward and back and must return, and the plane transpose must invert.  Test tooling, not part of librcx.so.
#include "predict_sim.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main()
{
    const u32 widths[3] = {2, 4, 8};
    for (u32 width : widths)
        for (u32 zigzag = 0; zigzag < 2; ++zigzag) {
            const u32 count = 1000;
            const size_t bytes = 16ull * width * count;
            std::vector<u8> in(bytes), out(bytes), back(bytes);
            std::vector<u64> fronts(count), totals(count);
            srand(width + zigzag);
            for (size_t i = 0; i < bytes; ++i) in[i] = (i / 64) % 3 == 0 ? 0xFF : (i / 64) % 3 == 1 ? 0 : (u8)rand();
            const u64 mask = width == 8 ? ~0ull : (1ull << (8 * width)) - 1;
            for (u32 i = 0; i < count; ++i) fronts[i] = i % 3 == 0 ? mask : i % 3 == 1 ? mask / 2 + 1 : ((((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand()) & mask);
            if (sim_predict_units(in.data(), fronts.data(), count, width, zigzag, out.data())) return 1;
            if (sim_unpredict_units(out.data(), fronts.data(), count, width, zigzag, back.data(), totals.data())) return 2;
            if (in != back) {
                printf("width %u zigzag %u: does not come back\n", width, zigzag);
                return 3;
            }
            if (!sim_planes_units(in.data(), count, width, out.data())) return 4;
            if (sim_unzigzag(sim_zigzag(mask, width), width) != mask || sim_unzigzag(sim_zigzag(mask / 2 + 1, width), width) != mask / 2 + 1) return 5;
        }
    printf("predict_san ok\n");
    return 0;
}
