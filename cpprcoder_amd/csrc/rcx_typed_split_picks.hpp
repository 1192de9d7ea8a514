// rcx_typed_split_picks.hpp -- the planner of rcx_typed_split_picks_device (include/rcx_typed_split_picks.h): what
// rcx_typed_plan(..., scan = false) does on the host (rcx_typed_items.hpp, whose comment block says what the tables must hold)
// for entries that lie in device memory, each with a source and a destination position of its own.  The mirror of
// rcx_typed_picks.hpp, and simpler: the forward predictor is local to an element and the one in front of it, so an entry with a
// predictor is an entry of its class like any other -- no scan list, no bins, no longest-first order, and nothing that has to be
// zero before the first launch.  Launches that follow one another:
//
//   rcx_spick_classify_k  entry k < min(*count, max_pick): validate it (rcx_tpick_validate, as it is) and give it a KEY: its
//                         class of rcx_typed_class (0 .. 11; 1 and 2 have no entries: width 1 takes no predictor), or none.
//                         Per tile of 256 entries the 12 classes' entries and whole units, packed as rcx_typed_picks.hpp packs
//                         them, and the bytes of all the tile's valid entries.
//   rcx_spick_top_k       one workgroup: the exclusive sums over the tiles for the 12 classes, from their totals the head of
//                         the tables (rcx_spick_head: RcxTypedClasses as rcx_typed_plan computes it without a scan list) and
//                         ufirst[nent]; the bytes against max_bytes -- above it the head is all zero, over[0] = 1 and
//                         RCX_E_CAPACITY latched at the count, so the walking kernel finds nothing to do.
//   rcx_spick_apply_k     the tiles of all max_pick entries: an entry takes place ent_first[class] + tile_ents + its rank in
//                         the tile -- the caller's order within the class, as the host plan has it -- and ufirst[place] =
//                         ubase[class] + tile_units + the units before it in the tile, an exact u64 prefix sum in the placed
//                         order; kept[k] = its length if it was placed, else 0, for every k < max_pick.
//   rcx_tpick_rows_k      (rcx_typed_picks.hpp, as it is) rowtab: the row rule reads only a head and a ufirst.
//
// Then rcx_typed_split_picks_k (rcx_typed_items.hpp) walks the tables.  No wave waits for another: what one launch leaves the
// next one reads.  Nothing is read behind min(*count, max_pick).  The 12 per-tile scans are rcx_base_picks.hpp's tile scan of 16
// keys, as it is: four scans of zeros more a tile in a planner that is bound by its table reads.
//
// The rules per entry are plain functions, also compiled into tests/sim/typed_split_picks_san.cpp.
#pragma once

#include "rcx_base_picks.hpp" // rcx_bpick_tile_scan, and through it rcx_typed_picks.hpp: rcx_tpick_validate, _units, _tiles, _row

#define RCX_SPICK_KEYS RCX_TYPED_CLASSES      // a valid entry's key is its class
#define RCX_SPICK_SUMS (RCX_SPICK_KEYS + 1u)  // a tile's sums: the 12 keys, then the bytes

// ---- the rules per entry: plain functions ----------------------------------------------------------------------------------
// rows of rowtab at the most when the valid entries have max_bytes between them: a unit has 16 bytes at least, a row 256 units,
// and each of the 12 classes one more row than whole ones and one closing entry: max_bytes / 4096 + 24 (rcx_bpick_rows_most's rule)
RCX_HD u64 rcx_spick_rows_most(u64 max_bytes) { return max_bytes / (16u * RCX_TYPED_ROW) + 2u * RCX_TYPED_CLASSES; }

// The head of the tables from the 12 classes' entries and whole units: what rcx_typed_plan(..., scan = false) computes.
RCX_HD void rcx_spick_head(const u64* nent12, const u64* units12, RcxTypedClasses& cl)
{
    u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c) {
        const u32 w = rcx_typed_class_width(c);
        const u64 n = nent12[c], un = units12[c];
        cl.ent_first[c] = (u32)ents;
        cl.row_first[c] = (u32)rows;
        cl.ubase[c] = ub;
        const u64 step = (u64)(RCX_PLANES_U4 / w) * RCX_TYPED_ROW;
        steps += (un + step - 1) / step;
        rests += (n * (17u * w) + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
        cl.step_end[c] = steps;
        cl.rest_end[c] = rests;
        ents += n;
        ub += un;
        if (n) rows += (un + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW + 1;
    }
    cl.ent_first[RCX_TYPED_CLASSES] = (u32)ents;
    cl.row_first[RCX_TYPED_CLASSES] = (u32)rows;
    cl.ubase[RCX_TYPED_CLASSES] = ub;
}

#if !defined(RCX_HOST_SIM)

static_assert(RCX_SPICK_KEYS <= RCX_BPICK_KEYS, "the tile scan has a sum for every class");

// The planned tables and the planner's own words, all in the context's table scratch (rcx_typed_split_picks_api.hpp has the
// layout).  What the call is given is an RcxTypedPickIn, as the join's; kept goes beside it.
struct RcxTypedSplitPickPlan {
    RcxTypedClasses* classes;
    u64* ufirst;     // [max_pick + 1]
    u64* from;       // [max_pick]
    u64* to;         // [max_pick]
    u64* tile_sum;   // [tiles][13]: classes 0 .. 11 (entries << 40 | units), bytes
    u64* tile_units; // [tiles][12]: the units of the class in the tiles before
    u32* tile_ents;  // [tiles][12]: the entries, likewise
    u32* len;        // [max_pick]
    u32* keys;       // [max_pick]
    u32* rowtab;     // [rcx_spick_rows_most(max_bytes)]
    u32* over;       // [2]: 1 if the bytes were above max_bytes; a zero word (what the walking kernel's tables name as nscan)
};

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_spick_classify_k(const RcxTypedPickIn t, const RcxTypedSplitPickPlan p, u32* status)
{
    __shared__ u64 lds[RCX_BPICK_KEYS][4];
    __shared__ u64 wave_bytes[4];
    const u64 count = rcx_tpick_count(t);
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.count[0] > t.max_pick) rcx_flag(status, RCX_ST_CAPACITY, t.max_pick);
    const u64 tiles = rcx_tpick_tiles(count);
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (whole workgroups go round)
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        u32 key = RCX_TPICK_NONE;
        u64 value = 0, bytes = 0;
        if (k < count) {
            const u64 len = t.len[k];
            if (len != 0) { // (a length of 0 is not looked at)
                const u32 w = t.widths[k], pr = t.preds ? t.preds[k] : 0u;
                const u32 bad = rcx_tpick_validate(t.src_at[k], t.dst_at[k], len, w, pr, t.src_cap, t.dst_cap);
                if (bad) {
                    rcx_flag(status, bad, k);
                } else {
                    key = rcx_typed_class(w, pr);
                    value = (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units((u32)len, w);
                    bytes = len;
                }
            }
            p.keys[k] = key;
        }
        u64 sum = bytes;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((threadIdx.x & 63u) == 0) wave_bytes[threadIdx.x >> 6] = sum;
        u64 before, total;
        rcx_bpick_tile_scan(key, value, lds, before, total); // (in step twice: wave_bytes is read behind the first)
        if (threadIdx.x < RCX_SPICK_KEYS) p.tile_sum[tile * RCX_SPICK_SUMS + threadIdx.x] = total;
        if (threadIdx.x == RCX_SPICK_KEYS) p.tile_sum[tile * RCX_SPICK_SUMS + RCX_SPICK_KEYS] = wave_bytes[0] + wave_bytes[1] + wave_bytes[2] + wave_bytes[3];
        __syncthreads(); // (wave_bytes is written again in the next turn)
    }
}

__global__ __launch_bounds__(RCX_TPICK_TOP) void rcx_spick_top_k(const RcxTypedPickIn t, const RcxTypedSplitPickPlan p, u32* status)
{
    __shared__ u64 lds[RCX_TPICK_TOP / 64u];
    __shared__ u64 totals[2 * RCX_SPICK_KEYS]; // the 12 classes' entries, then their units, for the one thread that writes the head
    const u64 count = rcx_tpick_count(t), tiles = rcx_tpick_tiles(count);
    u64 bytes = 0;
    for (u32 c = 0; c < RCX_SPICK_KEYS; ++c) { // (a loop, not unrolled: one class's sums over all tiles at a time)
        u64 ents = 0, units = 0; // of the tiles before this pass (the same in every thread)
        for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
            const u64 tile = base + threadIdx.x;
            const bool has = tile < tiles;
            const u64 v = has ? p.tile_sum[tile * RCX_SPICK_SUMS + c] : 0ull;
            const u64 n = v >> RCX_TPICK_COUNT_SHIFT, un = v & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull);
            u64 all_n, all_un;
            const u64 upto_n = rcx_tpick_top_scan<u64>(n, lds, all_n), upto_un = rcx_tpick_top_scan<u64>(un, lds, all_un);
            if (has) {
                p.tile_ents[tile * RCX_SPICK_KEYS + c] = (u32)(ents + upto_n - n);
                p.tile_units[tile * RCX_SPICK_KEYS + c] = units + upto_un - un;
            }
            ents += all_n;
            units += all_un;
        }
        if (threadIdx.x == 0) {
            totals[c] = ents;
            totals[RCX_SPICK_KEYS + c] = units;
        }
    }
    for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
        const u64 tile = base + threadIdx.x;
        u64 all_bytes;
        (void)rcx_tpick_top_scan<u64>(tile < tiles ? p.tile_sum[tile * RCX_SPICK_SUMS + RCX_SPICK_KEYS] : 0ull, lds, all_bytes);
        bytes += all_bytes;
    }
    const bool over = bytes > t.max_bytes;
    if (threadIdx.x == 0) { // (totals[] is this thread's own writing)
        if (over) {
            rcx_flag(status, RCX_ST_CAPACITY, count);
            for (u32 c = 0; c < 2 * RCX_SPICK_KEYS; ++c) totals[c] = 0;
        }
        RcxTypedClasses& cl = *p.classes;
        rcx_spick_head(totals, totals + RCX_SPICK_KEYS, cl);
        p.ufirst[cl.ent_first[RCX_TYPED_CLASSES]] = cl.ubase[RCX_TYPED_CLASSES];
        p.over[0] = over ? 1u : 0u;
        p.over[1] = 0u;
    }
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_spick_apply_k(const RcxTypedPickIn t, const RcxTypedSplitPickPlan p, u64* kept)
{
    __shared__ u64 lds[RCX_BPICK_KEYS][4];
    const u64 count = rcx_tpick_count(t), tiles = rcx_tpick_tiles(t.max_pick); // (every entry's kept is written, also behind the count)
    const RcxTypedClasses* const cl = p.classes;
    const bool over = p.over[0] != 0u;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        const u32 key = k < count && !over ? p.keys[k] : RCX_TPICK_NONE;
        const bool live = key != RCX_TPICK_NONE;
        const u32 len = live ? (u32)t.len[k] : 0u;
        const u32 w = live ? t.widths[k] : 1u;
        const u64 value = live ? (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units(len, w) : 0ull;
        u64 before, total;
        rcx_bpick_tile_scan(key, value, lds, before, total);
        bool placed = false;
        if (live) {
            const u64 place = (u64)cl->ent_first[key] + p.tile_ents[tile * RCX_SPICK_KEYS + key] + (before >> RCX_TPICK_COUNT_SHIFT);
            if (place < t.max_pick) { // (it is: the classes hold at most `count` entries between them)
                p.ufirst[place] = cl->ubase[key] + p.tile_units[tile * RCX_SPICK_KEYS + key] + (before & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull));
                p.from[place] = t.src_at[k];
                p.to[place] = t.dst_at[k];
                p.len[place] = len;
                placed = true;
            }
        }
        if (kept && k < t.max_pick) kept[k] = placed ? (u64)len : 0ull;
    }
}

#endif // !RCX_HOST_SIM
