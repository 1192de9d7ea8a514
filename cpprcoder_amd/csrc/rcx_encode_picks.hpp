// rcx_encode_picks.hpp -- the planner of rcx_encode_picks_device (include/rcx_encode_picks.h): what plan_items does on the host
// (rcx_items.hpp) for an encode call whose tables are in device memory.  Four kernels, one launch each, and the size scan:
//
//   rcx_epicks_clear_k      bins[] = 0, the byte total = 0 (a kernel, not a memset: rcx_picks.hpp)
//   rcx_epicks_classify_k   entry k < min(*d_count, max_items): validate it (the rules of the header, in their order) and give
//                           it a BIN or none; bins[] counts the entries of every bin, the lengths of the valid entries are
//                           added up.  keys[k] = the bin, inv[k] = none, for every k < max_items.
//   rcx_epicks_scan_k       one workgroup: the layout.  The bins in work order (longest first) fall into 21 length CLASSES --
//                           the power of two at or above the length, at least 16, what plan_items calls item_class_upper --
//                           and every class begins on a multiple of 64 work positions, a UNIT (rcx_geom.hpp, RcxEncPicks):
//                           cursor[b] = the position of bin b's first entry, unit[u] = {stride of the class, where the unit's
//                           slots begin}, the positions behind a class's last entry up to the next unit are HOLES (length 0),
//                           counts[0] = the positions laid out.  A total above max_bytes: counts[0] = 0, counts[1] = 1 and the
//                           failure is latched; nothing is encoded.
//   rcx_epicks_scatter_k    entry k with a bin takes the next place of its bin and writes {at, len, id} there and inv[k].
//   rcx_epicks_sizes_k      rcx_scan_sizes_k for max_items table entries, the failure reported at the device's count.
//
// The bin of an entry is rcx_pick_bin (rcx_picks.hpp) of its length - 1, not of its length: a class is (U / 2, U], so the
// lengths U and U + 1 lie in different classes, and above 512 rcx_pick_bin gives both the same bin (the same leading one,
// the same eight bits behind it).  Of length - 1 the classes are [U / 2, U - 1] -- one leading bit -- and no bin spans two.
// A slot base is a sum over the live entries in front, holes take no slot memory; the slots of a class lie in one piece.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_picks.hpp"

#define RCX_EPICK_CLASSES 21u // uppers 2^24 (as RCX_MAX_BLOCK), 2^23, ... 16: longest first
#define RCX_EPICK_BINS RCX_PICK_CODED_BINS
#define RCX_EPICK_PAD (64u * (RCX_EPICK_CLASSES + 1u)) // work positions beyond max_items: a unit's padding per class, the launch's

// the upper length of class c (what item_class_upper gives its lengths), and the bin of a length 1 .. RCX_MAX_BLOCK
RCX_HD u32 rcx_epick_upper(u32 c)
{
    const u32 up = 1u << (24u - c);
    return up > RCX_MAX_BLOCK ? RCX_MAX_BLOCK : up;
}
RCX_HD u32 rcx_epick_bin(u32 len) { return rcx_pick_bin(len - 1u); }

// What the call is given, as the kernels take it.
struct RcxEpickTables {
    const u64* src_at;
    const u64* src_len;
    const u64* count;
    u64 src_cap, max_items, max_bytes, positions; // positions: what the tables of the plan have room for
    u32 max_len;
};

// What the host knows of the classes: where each one's bins begin (first_bin[21] = the end) and its slots' stride.
struct RcxEpickClasses {
    u32 first_bin[RCX_EPICK_CLASSES + 1];
    u32 stride[RCX_EPICK_CLASSES];
};

// The planned tables (RcxEncPicks) and the planner's own words, all in the context's table scratch.
struct RcxEpickPlan {
    u64* at;          // [positions]
    u64* total;       // [2]: the valid entries' bytes
    RcxEncUnit* unit; // [positions / 64 + 1]
    u32* len;         // [positions]
    u32* id;          // [positions]
    u32* inv;         // [max_items]
    u32* keys;        // [max_items]
    u32* cursor;      // [RCX_EPICK_BINS]
    u32* bins;        // [RCX_EPICK_BINS], zero when the classify kernel starts
    u32* counts;      // [4]: positions laid out (a multiple of 64), 1 = the total is above max_bytes
};

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_epicks_clear_k(const RcxEpickPlan p)
{
    const u32 b = blockIdx.x * RCX_PICK_THREADS + threadIdx.x;
    if (b < RCX_EPICK_BINS) p.bins[b] = 0;
    if (b == 0) p.total[0] = 0;
}

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_epicks_classify_k(const RcxEpickTables t, const RcxEpickPlan p, u32* status)
{
    const u64 count = rcx_pick_count(t.count, t.max_items);
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.count[0] > t.max_items) rcx_flag(status, RCX_ST_CAPACITY, t.max_items);
    u64 bytes = 0;
    // whole waves: every lane of a wave that has a table entry goes round
    for (u64 k0 = (u64)blockIdx.x * RCX_PICK_THREADS; k0 < t.max_items; k0 += (u64)gridDim.x * RCX_PICK_THREADS) {
        const u64 k = k0 + threadIdx.x;
        u32 bin = RCX_PICK_NONE;
        if (k < count) {
            const u64 len = t.src_len[k];
            if (len != 0) { // (a length of 0 is not looked at)
                const u64 at = t.src_at[k];
                if (len > (u64)t.max_len) {
                    rcx_flag(status, RCX_ST_CORRUPT, k);
                } else if (at > t.src_cap || len > t.src_cap - at) {
                    rcx_flag(status, RCX_ST_CAPACITY, k);
                } else {
                    bin = rcx_epick_bin((u32)len);
                    bytes += len;
                }
            }
        }
        if (k < t.max_items) {
            p.keys[k] = bin;
            p.inv[k] = RCX_PICK_NONE;
        }
        (void)rcx_pick_take(p.bins, bin, bin != RCX_PICK_NONE);
    }
    // (at most 2^31 entries of less than 2^24 bytes: no wrap)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bytes += (u64)__shfl_xor((unsigned long long)bytes, o, 64);
    if ((threadIdx.x & 63u) == 0 && bytes != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.total), (unsigned long long)bytes);
}

__global__ __launch_bounds__(RCX_PICK_SCAN_THREADS) void rcx_epicks_scan_k(const RcxEpickTables tb, const RcxEpickPlan p, const RcxEpickClasses cl, u32* status)
{
    __shared__ u32 lds[RCX_PICK_SCAN_THREADS / 64u];
    __shared__ u32 pre[RCX_EPICK_BINS + 1];        // entries in the bins before b
    __shared__ u32 cstart[RCX_EPICK_CLASSES + 1];  // the class's first work position; [21] = the positions laid out
    __shared__ u64 cbase[RCX_EPICK_CLASSES];       // where its slots begin
    __shared__ u32 over;
    const u32 t = threadIdx.x;
    const u32 all = rcx_bins_scan<RCX_EPICK_BINS>(p.bins, lds, [&](u32 b, u32 before, u32) { pre[b] = before; });
    if (t == 0) pre[RCX_EPICK_BINS] = all;
    __syncthreads();
    if (t == 0) {
        u32 pos = 0;
        u64 base = 0;
        for (u32 c = 0; c < RCX_EPICK_CLASSES; ++c) {
            const u32 n = pre[cl.first_bin[c + 1]] - pre[cl.first_bin[c]];
            cstart[c] = pos;
            cbase[c] = base;
            pos += (n + 63u) & ~63u;
            base += (u64)n * cl.stride[c];
        }
        cstart[RCX_EPICK_CLASSES] = pos;
        const bool too_many = p.total[0] > tb.max_bytes;
        over = too_many ? 1u : 0u;
        p.counts[0] = too_many ? 0u : pos;
        p.counts[1] = over;
        if (too_many) rcx_flag(status, RCX_ST_CAPACITY, rcx_pick_count(tb.count, tb.max_items));
    }
    __syncthreads();
    if (over) return; // (every thread: nothing of the layout is read)
    for (u32 b = t; b < RCX_EPICK_BINS; b += RCX_PICK_SCAN_THREADS) {
        u32 c = 0;
        while (b >= cl.first_bin[c + 1]) ++c; // (first_bin[21] = RCX_EPICK_BINS)
        p.cursor[b] = cstart[c] + (pre[b] - pre[cl.first_bin[c]]);
    }
    const u32 laid = cstart[RCX_EPICK_CLASSES];
    for (u32 u = t; u < laid / 64u; u += RCX_PICK_SCAN_THREADS) {
        u32 c = 0;
        while (64u * u >= cstart[c + 1]) ++c; // (an empty class begins where the next one does and is passed over)
        p.unit[u] = RcxEncUnit{cbase[c] + (u64)(64u * u - cstart[c]) * cl.stride[c], cl.stride[c], 0u};
    }
    for (u32 i = t; i < 64u * RCX_EPICK_CLASSES; i += RCX_PICK_SCAN_THREADS) { // the holes behind every class
        const u32 c = i >> 6;
        const u32 n = pre[cl.first_bin[c + 1]] - pre[cl.first_bin[c]];
        const u32 w = cstart[c] + n + (i & 63u);
        if (w < cstart[c + 1]) p.len[w] = 0;
    }
}

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_epicks_scatter_k(const RcxEpickTables t, const RcxEpickPlan p)
{
    if (p.counts[1]) return;
    const u64 count = rcx_pick_count(t.count, t.max_items);
    for (u64 k0 = (u64)blockIdx.x * RCX_PICK_THREADS; k0 < count; k0 += (u64)gridDim.x * RCX_PICK_THREADS) {
        const u64 k = k0 + threadIdx.x;
        const u32 bin = k < count ? p.keys[k] : RCX_PICK_NONE;
        const bool has = bin != RCX_PICK_NONE;
        const u32 w = rcx_pick_take(p.cursor, bin, has);
        if (has && (u64)w < t.positions) { // (the layout holds at most count + 63 * 21 positions)
            p.at[w] = t.src_at[k];
            p.len[w] = (u32)t.src_len[k];
            p.id[w] = (u32)k;
            p.inv[k] = w;
        }
    }
}

// rcx_scan_sizes_k (rcx_kernels.hpp) over the max_items entries of the offsets table -- an entry without a work position has
// size 0 -- with the failure at the device's count, where the host-planned call reports it at its item count.
__global__ __launch_bounds__(1024) void rcx_epicks_sizes_k(const u32* __restrict__ sizes, const u64* __restrict__ count, u64 max_items,
                                                           u64* __restrict__ offsets, u64 dst_cap, u32* status, const RcxEncPicks g)
{
    __shared__ u64 wave_total[16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 per = (max_items + 1023) / 1024;
    const u64 first = (u64)tid * per;
    const u64 last = (first + per) < max_items ? (first + per) : max_items;
    u64 mine = 0;
    for (u64 b = first; b < last; ++b) mine += rcx_size_of(g, sizes, b);
    u64 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u64 up = (u64)__shfl_up((unsigned long long)incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    u64 before = 0;
    for (u32 w = 0; w < wave; ++w) before += wave_total[w];
    u64 run = before + incl - mine;
    for (u64 b = first; b < last; ++b) {
        offsets[b] = run;
        run += rcx_size_of(g, sizes, b);
    }
    if (tid == 1023) {
        offsets[max_items] = before + incl;
        if (before + incl > dst_cap) rcx_flag(status, RCX_ST_CAPACITY, count[0] < max_items ? count[0] : max_items);
    }
}
