// predict_sim.cpp -- the per-unit arithmetic of cpprcoder_amd/csrc/rcx_predict.hpp compiled for the host (g++, no HIP), so
// that tests/test_predict_cpu.py can hold it against a scalar loop before it meets a GPU.  Test tooling: not part of
// librcx.so.  A unit is 16 elements of W bytes, handed over as 16 * W bytes in memory order.
#include <string.h>

#include "../../cpprcoder_amd/csrc/rcx_predict.hpp"

uint64_t rcx_sim_counters[4];

namespace
{

template <u32 W, bool ZIGZAG>
void forward(const u8* in, u64 prev, u8* out)
{
    u32 w[4 * W], o[4 * W];
    memcpy(w, in, 16 * W);
    rcx_predict_unit<W, ZIGZAG>(w, (typename RcxElem<W>::T)prev, o);
    memcpy(out, o, 16 * W);
}

// -> the unit's total (what the wave scan is handed)
template <u32 W, bool ZIGZAG>
u64 inverse(const u8* in, u64 before, u8* out)
{
    typedef typename RcxElem<W>::T T;
    u32 w[4 * W], o[4 * W];
    T e[16];
    memcpy(w, in, 16 * W);
    rcx_unpredict_scan<W, ZIGZAG>(w, e);
    rcx_unpredict_finish<W>(e, (T)before, o);
    memcpy(out, o, 16 * W);
    return e[15];
}

// split then join of the planes is the identity, and split is the transpose
template <u32 W>
int planes(const u8* in, u8* planes_out)
{
    u32 w[4 * W], o[4 * W], back[4 * W];
    memcpy(w, in, 16 * W);
    rcx_planes_unit<W, false>(w, o);
    rcx_planes_unit<W, true>(o, back);
    memcpy(planes_out, o, 16 * W);
    return memcmp(w, back, 16 * W) == 0;
}

} // namespace

extern "C" {

// `count` units back to back; unit k's element in front is prevs[k].  0 = done, -1 = no such width.
int sim_predict_units(const u8* in, const u64* prevs, u32 count, u32 width, u32 zigzag, u8* out)
{
    for (u32 k = 0; k < count; ++k) {
        const u8* a = in + 16ull * width * k;
        u8* b = out + 16ull * width * k;
        if (width == 2) zigzag ? forward<2, true>(a, prevs[k], b) : forward<2, false>(a, prevs[k], b);
        else if (width == 4) zigzag ? forward<4, true>(a, prevs[k], b) : forward<4, false>(a, prevs[k], b);
        else if (width == 8) zigzag ? forward<8, true>(a, prevs[k], b) : forward<8, false>(a, prevs[k], b);
        else return -1;
    }
    return 0;
}

// The inverse of the above: unit k's sum of everything in front is befores[k]; totals[k] = the unit's own total.
int sim_unpredict_units(const u8* in, const u64* befores, u32 count, u32 width, u32 zigzag, u8* out, u64* totals)
{
    for (u32 k = 0; k < count; ++k) {
        const u8* a = in + 16ull * width * k;
        u8* b = out + 16ull * width * k;
        if (width == 2) totals[k] = zigzag ? inverse<2, true>(a, befores[k], b) : inverse<2, false>(a, befores[k], b);
        else if (width == 4) totals[k] = zigzag ? inverse<4, true>(a, befores[k], b) : inverse<4, false>(a, befores[k], b);
        else if (width == 8) totals[k] = zigzag ? inverse<8, true>(a, befores[k], b) : inverse<8, false>(a, befores[k], b);
        else return -1;
    }
    return 0;
}

// One element through zigzag and back.
u64 sim_zigzag(u64 d, u32 width)
{
    return width == 2 ? rcx_zigzag<2>((u32)d) : width == 4 ? rcx_zigzag<4>((u32)d) : rcx_zigzag<8>(d);
}

u64 sim_unzigzag(u64 z, u32 width)
{
    return width == 2 ? rcx_unzigzag<2>((u32)z) : width == 4 ? rcx_unzigzag<4>((u32)z) : rcx_unzigzag<8>(z);
}

// The plane transpose of `count` units: 1 if every unit also came back from join(split()).
int sim_planes_units(const u8* in, u32 count, u32 width, u8* out)
{
    int ok = 1;
    for (u32 k = 0; k < count; ++k) {
        const u8* a = in + 16ull * width * k;
        u8* b = out + 16ull * width * k;
        ok &= width == 2 ? planes<2>(a, b) : width == 4 ? planes<4>(a, b) : planes<8>(a, b);
    }
    return ok;
}

} // extern "C"
