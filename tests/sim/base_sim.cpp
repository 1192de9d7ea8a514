// base_sim.cpp -- the per-unit arithmetic of cpprcoder_amd/csrc/rcx_base.hpp compiled for the host (g++, no HIP) as a program
// of its own, to be built with -fsanitize=address,undefined (tests/test_base_cpu.py does), so that the word arithmetic -- the
// borrow-free byte formulas, the 16-bit lanes, the word pairs of width 8 -- meets the numpy twin before it meets a GPU.
// Test tooling: not part of librcx.so.
//
//     base_sim WIDTH OP JOIN SRC BASE OUT
// SRC and BASE hold the same number of units of 16 elements (16 * WIDTH bytes each, memory order).  Every unit goes through
// what a lane of rcx_base_k does with it: split (JOIN = 0) = rcx_base_unit, then rcx_planes_unit for WIDTH > 1; join = the
// other way round.  That is the transform of include/rcx_base.h at block = 16, where every unit is a superblock.  Beside it
// every element goes through the scalar rcx_base_elem, which the lanes behind the unit loop use, and the two must agree.
// Exit status 0 = OUT written; 2 = usage or files; 3 = word arithmetic and scalar statement disagree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cpprcoder_amd/csrc/rcx_base.hpp"

uint64_t rcx_sim_counters[4];

namespace
{

template <u32 W, u32 OP, bool JOIN>
int unit(const u8* in, const u8* base, u8* out)
{
    u32 w[4 * W], b[4 * W], r[4 * W], o[4 * W], elements_in[4 * W], elements_out[4 * W];
    memcpy(w, in, 16 * W);
    memcpy(b, base, 16 * W);
    if constexpr (W == 1) {
        rcx_base_unit<W, OP, JOIN>(w, b, o);
        memcpy(elements_in, w, 16 * W);
        memcpy(elements_out, o, 16 * W);
    } else if (JOIN) {
        rcx_planes_unit<W, true>(w, r);
        rcx_base_unit<W, OP, true>(r, b, o);
        memcpy(elements_in, r, 16 * W);
        memcpy(elements_out, o, 16 * W);
    } else {
        rcx_base_unit<W, OP, false>(w, b, r);
        rcx_planes_unit<W, false>(r, o);
        memcpy(elements_in, w, 16 * W);
        memcpy(elements_out, r, 16 * W);
    }
    memcpy(out, o, 16 * W);
    // the scalar statement, element by element (before the transpose on the way in, behind it on the way out)
    const u8 *ei = reinterpret_cast<const u8*>(elements_in), *eo = reinterpret_cast<const u8*>(elements_out);
    for (u32 k = 0; k < 16; ++k) {
        u64 x = 0, y = 0, got = 0;
        memcpy(&x, ei + k * W, W);
        memcpy(&y, base + k * W, W);
        memcpy(&got, eo + k * W, W);
        if (rcx_base_elem<W, OP, JOIN>(x, y) != got) return 3;
    }
    return 0;
}

template <u32 W, u32 OP>
int units(bool join, const std::vector<u8>& in, const std::vector<u8>& base, std::vector<u8>& out)
{
    for (size_t at = 0; at + 16 * W <= in.size(); at += 16 * W) {
        const int r = join ? unit<W, OP, true>(&in[at], &base[at], &out[at]) : unit<W, OP, false>(&in[at], &base[at], &out[at]);
        if (r) return r;
    }
    return 0;
}

template <u32 W>
int ops(u32 op, bool join, const std::vector<u8>& in, const std::vector<u8>& base, std::vector<u8>& out)
{
    return op == 0 ? units<W, 0>(join, in, base, out) : op == 1 ? units<W, 1>(join, in, base, out) : units<W, 2>(join, in, base, out);
}

bool slurp(const char* path, std::vector<u8>& to)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    u8 chunk[4096];
    for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) to.insert(to.end(), chunk, chunk + got);
    fclose(f);
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const u32 width = (u32)atoi(argv[1]), op = (u32)atoi(argv[2]);
    const bool join = atoi(argv[3]) != 0;
    std::vector<u8> in, base;
    if (!slurp(argv[4], in) || !slurp(argv[5], base) || in.size() != base.size() || op > 2) return 2;
    if (!(width == 1 || width == 2 || width == 4 || width == 8) || in.size() % (16 * width)) return 2;
    std::vector<u8> out(in.size());
    const int r = width == 1 ? ops<1>(op, join, in, base, out) : width == 2 ? ops<2>(op, join, in, base, out) : width == 4 ? ops<4>(op, join, in, base, out)
                                                                                                                          : ops<8>(op, join, in, base, out);
    if (r) return r;
    FILE* f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("base_sim ok: %zu units\n", in.size() / (16 * width));
    return 0;
}
