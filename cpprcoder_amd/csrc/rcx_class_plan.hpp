// rcx_class_plan.hpp -- the class planner: the one planner of the typed join (rcx_typed_picks.hpp), the base join
// (rcx_base_picks.hpp) and the typed split (rcx_typed_split_picks.hpp) over entries that lie in device memory.  Included by
// rcx_typed_picks.hpp behind its constants and its rules per entry; a call's own part is a POLICY:
//
//   In                  what the call is given: src_at, dst_at, len, widths, preds, count, max_pick, max_bytes and its own
//   KEYS                the class keys; a valid entry has a key below KEYS, or KEYS + its bin in the scan list
//   classify(t, k, len, w, key)   validate entry k (len > 0 bytes, width w) -> RCX_TPICK_OK and its key, or what it is skipped with
//   SETS, set_of(key), class_of(key), rows(set, w)   the set of tables (RcxClassSet) and the class of rcx_typed_class a key
//                       lands in, and the rows of a workgroup step of the set's walking kernel
//   SCAN                there is a scan list: bins, cursor, nscan[0] and the clear launch in front
//   KEPT                kept[k] = the length of entry k if it was placed, else 0, for every k < max_pick
//
// Launches that follow one another; no wave waits for another, what one launch leaves the next one reads:
//
//   rcx_class_clear_k     (SCAN) bins[] = 0, by a kernel: a captured call is kernel nodes alone.
//   rcx_class_classify_k  entry k < min(*count, max_pick): validate it and give it its key or none.  A TILE is the 256 entries
//                         of a workgroup's turn; tile_sum[tile] = per key the entries and their whole units (entries << 40 |
//                         units), and the bytes of all the tile's valid entries.  bins[] counts the scan list's bins, a wave at
//                         a time (rcx_pick_take).
//   rcx_class_top_k       one workgroup, 1024 tiles a pass, a key at a time: the exclusive sums over the tiles (tile_ents,
//                         tile_units), from their totals the head of every set (rcx_class_head) and its closing ufirst; the
//                         bytes against max_bytes -- above it every head is all zero, nscan = {0, 1} and RCX_E_CAPACITY latched
//                         at the count, so the walking kernels find nothing to do; the bins' cursors (rcx_bins_scan).
//   rcx_class_apply_k     the tiles again: an entry with a key below KEYS takes place ent_first[class] + tile_ents + its rank
//                         in the tile -- the caller's order within the class, as the host plan has it -- and ufirst[place] =
//                         ubase[class] + tile_units + the units before it in the tile, an exact u64 prefix sum in the placed
//                         order; an entry of the scan list takes the next place of its bin.  Nothing is placed when the bytes
//                         were above max_bytes.
//   rcx_class_rows_k      once a set: rowtab, row r of a class = the entry of unit ubase + 256 r, by bisection over the
//                         class's entries (rcx_typed_locate, the kernels' own search), and the class's last entry once more.
//
// The sums are exact (u64 units, u32 entries).  Nothing is read behind min(*count, max_pick).  The head and the row rule are
// plain functions, also compiled into tests/sim/*_picks_san.cpp.
#pragma once
#if !defined(RCX_TPICK_THREADS)
#error "rcx_class_plan.hpp is included through rcx_typed_picks.hpp, which has its constants"
#endif

// One set's tables, as its walking kernel reads them.
struct RcxClassSet {
    RcxTypedClasses* classes; // the head
    u64* ufirst;              // [max_pick + 1]
    u64* from;                // [max_pick]
    u64* to;                  // [max_pick]
    u32* len;                 // [max_pick]
    u32* rowtab;              // [rcx_class_rows_most]
    u64* bat;                 // [max_pick] the entry's offset in the base, or nullptr: the set has none
};

// rows of a set's rowtab at the most when the valid entries have max_bytes between them and `classes` of the 12 classes can
// have entries: a unit has 16 bytes at least, a row 256 units, every class one more row than whole ones and one closing entry
RCX_HD u64 rcx_class_rows_most(u64 max_bytes, u32 classes) { return max_bytes / (16u * RCX_TYPED_ROW) + 2u * classes; }

// The head of a set from its 12 classes' entries and whole units: what rcx_typed_plan and rcx_base_items_plan compute.
// rows_of(w) = the rows of a workgroup step of width w.
template <class Rows>
RCX_HD void rcx_class_head(const u64* nent12, const u64* units12, Rows rows_of, RcxTypedClasses& cl)
{
    u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c) {
        const u32 w = rcx_typed_class_width(c);
        const u64 n = nent12[c], un = units12[c];
        cl.ent_first[c] = (u32)ents;
        cl.row_first[c] = (u32)rows;
        cl.ubase[c] = ub;
        const u64 step = (u64)rows_of(w) * RCX_TYPED_ROW;
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

// Row r of rowtab (r below row_first[RCX_TYPED_CLASSES]): the entry of the row's first unit, or the class's last entry for
// the row that closes the class.
RCX_DEV u32 rcx_class_row(const RcxTypedClasses& cl, const u64* ufirst, u32 r)
{
    u32 c = 0;
    while (r >= cl.row_first[c + 1]) ++c;
    const u32 local = r - cl.row_first[c], nrow = cl.row_first[c + 1] - cl.row_first[c] - 1u;
    const u32 first = cl.ent_first[c], last = cl.ent_first[c + 1] - 1u;
    if (local == nrow) return last;
    return rcx_typed_locate(ufirst, first, last, cl.ubase[c] + (u64)local * RCX_TYPED_ROW);
}

#if !defined(RCX_HOST_SIM)

#include "rcx_picks.hpp" // rcx_pick_take, rcx_pick_count, rcx_group_scan, rcx_bins_scan

static_assert(RCX_TPICK_TOP == RCX_PICK_SCAN_THREADS, "rcx_group_scan is over the top workgroup");

// The planned tables and the planner's own words, all in the context's table scratch (rcx_typed_picks_api.hpp has the layout).
struct RcxClassPlan {
    RcxClassSet set[2]; // the policy's SETS of them
    u64* tile_sum;      // [tiles][KEYS + 1]: the keys (entries << 40 | units), bytes
    u64* tile_units;    // [tiles][KEYS]: the units of the key in the tiles before
    u32* tile_ents;     // [tiles][KEYS]: the entries, likewise
    u32* keys;          // [max_pick]
    u32* nscan;         // [2]: the scan list's length; 1 if the bytes were above max_bytes
    u64* scan_from;     // [max_pick], and what follows: with a scan list only
    u64* scan_to;       // [max_pick]
    u32* scan_len;      // [max_pick]
    u8* scan_kind;      // [max_pick]
    u32* cursor;        // [RCX_TPICK_BINS]
    u32* bins;          // [RCX_TPICK_BINS], zero when the classify kernel starts
};

// A tile's sums: every thread of the workgroup gives its key (below KEYS, or anything else: no class) and its value
// (1 << 40 | units).  before = what the threads below it gave to ITS key, total_mine: thread c < KEYS gets the tile's total of
// key c.  lds: KEYS x 4 words; ends with the workgroup in step, so that lds may be used again.
template <u32 KEYS>
__device__ __forceinline__ void rcx_class_tile_scan(u32 key, u64 value, u64 (*lds)[4], u64& before, u64& total_mine)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 mine = 0; // the inclusive sum of the thread's own key in its wave
#pragma unroll
    for (u32 c = 0; c < KEYS; ++c) {
        const u64 upto = rcx_wave_scan<u64>(key == c ? value : 0ull, lane);
        if (lane == 63u) lds[c][wave] = upto;
        if (key == c) mine = upto;
    }
    __syncthreads();
    before = 0;
    const u32 c_total = threadIdx.x < KEYS ? threadIdx.x : 0u;
    total_mine = lds[c_total][0] + lds[c_total][1] + lds[c_total][2] + lds[c_total][3];
    if (key < KEYS) {
        u64 front = 0;
#pragma unroll
        for (u32 w = 0; w < 4; ++w) front += w < wave ? lds[key][w] : 0ull;
        before = front + mine - value;
    }
    __syncthreads();
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_class_clear_k(const RcxClassPlan p)
{
    const u32 b = blockIdx.x * RCX_TPICK_THREADS + threadIdx.x;
    if (b < RCX_TPICK_BINS) p.bins[b] = 0;
    if (b < 2u) p.nscan[b] = 0;
}

template <class P>
__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_class_classify_k(const typename P::In t, const RcxClassPlan p, u32* status)
{
    constexpr u32 KEYS = P::KEYS, SUMS = KEYS + 1u;
    __shared__ u64 lds[KEYS][4];
    __shared__ u64 wave_bytes[4];
    const u64 count = rcx_pick_count(t.count, t.max_pick);
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.count[0] > t.max_pick) rcx_flag(status, RCX_ST_CAPACITY, t.max_pick);
    const u64 tiles = rcx_tpick_tiles(count);
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (whole workgroups go round)
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        u32 key = RCX_TPICK_NONE;
        u64 value = 0, bytes = 0;
        if (k < count) {
            const u64 len = t.len[k];
            if (len != 0) { // (a length of 0 is not looked at)
                const u32 w = t.widths[k];
                u32 mine = RCX_TPICK_NONE;
                const u32 bad = P::classify(t, k, len, w, mine);
                if (bad) {
                    rcx_flag(status, bad, k);
                } else {
                    key = mine;
                    value = (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units((u32)len, w);
                    bytes = len;
                }
            }
            p.keys[k] = key;
        }
        if constexpr (P::SCAN) (void)rcx_pick_take(p.bins, key - KEYS, key != RCX_TPICK_NONE && key >= KEYS);
        // the bytes of the tile
        u64 sum = bytes;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((threadIdx.x & 63u) == 0) wave_bytes[threadIdx.x >> 6] = sum;
        u64 before, total;
        rcx_class_tile_scan<KEYS>(key, value, lds, before, total); // (in step twice: wave_bytes is read behind the first)
        if (threadIdx.x < KEYS) p.tile_sum[tile * SUMS + threadIdx.x] = total;
        if (threadIdx.x == KEYS) p.tile_sum[tile * SUMS + KEYS] = wave_bytes[0] + wave_bytes[1] + wave_bytes[2] + wave_bytes[3];
        __syncthreads(); // (wave_bytes is written again in the next turn)
    }
}

template <class P>
__global__ __launch_bounds__(RCX_TPICK_TOP) void rcx_class_top_k(const typename P::In t, const RcxClassPlan p, u32* status)
{
    constexpr u32 KEYS = P::KEYS, SUMS = KEYS + 1u, NC = RCX_TYPED_CLASSES;
    __shared__ u64 lds[RCX_TPICK_TOP / 64u];
    __shared__ u32 lds32[RCX_TPICK_TOP / 64u];
    __shared__ u64 totals[2 * KEYS]; // the keys' entries, then their units, for the one thread that writes the heads
    __shared__ u64 of_class[2 * NC]; // a set's 12 classes likewise
    const u64 count = rcx_pick_count(t.count, t.max_pick), tiles = rcx_tpick_tiles(count);
    u64 bytes = 0;
    for (u32 c = 0; c < KEYS; ++c) { // (a loop, not unrolled: one key's sums over all tiles at a time)
        u64 ents = 0, units = 0; // of the tiles before this pass (the same in every thread)
        for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
            const u64 tile = base + threadIdx.x;
            const bool has = tile < tiles;
            const u64 v = has ? p.tile_sum[tile * SUMS + c] : 0ull;
            const u64 n = v >> RCX_TPICK_COUNT_SHIFT, un = v & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull);
            u64 all_n, all_un;
            const u64 upto_n = rcx_group_scan<u64>(n, lds, all_n), upto_un = rcx_group_scan<u64>(un, lds, all_un);
            if (has) {
                p.tile_ents[tile * KEYS + c] = (u32)(ents + upto_n - n);
                p.tile_units[tile * KEYS + c] = units + upto_un - un;
            }
            ents += all_n;
            units += all_un;
        }
        if (threadIdx.x == 0) {
            totals[c] = ents;
            totals[KEYS + c] = units;
        }
    }
    for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
        const u64 tile = base + threadIdx.x;
        u64 all_bytes;
        (void)rcx_group_scan<u64>(tile < tiles ? p.tile_sum[tile * SUMS + KEYS] : 0ull, lds, all_bytes);
        bytes += all_bytes;
    }
    const bool over = bytes > t.max_bytes;
    if (threadIdx.x == 0) { // (totals[] and of_class[] are this thread's own writing)
        if (over) rcx_flag(status, RCX_ST_CAPACITY, count);
        for (u32 s = 0; s < P::SETS; ++s) {
            for (u32 c = 0; c < 2 * NC; ++c) of_class[c] = 0;
            for (u32 key = 0; key < KEYS; ++key) {
                if (over || P::set_of(key) != s) continue;
                of_class[P::class_of(key)] = totals[key];
                of_class[NC + P::class_of(key)] = totals[KEYS + key];
            }
            RcxTypedClasses& cl = *p.set[s].classes;
            rcx_class_head(of_class, of_class + NC, [s](u32 w) { return P::rows(s, w); }, cl);
            p.set[s].ufirst[cl.ent_first[NC]] = cl.ubase[NC];
        }
        p.nscan[0] = 0u; // (with a scan list: its length, below)
        p.nscan[1] = over ? 1u : 0u;
    }
    if constexpr (P::SCAN) { // the scan list: cursor[b] = the entries of the bins before b
        const u32 all = rcx_bins_scan<RCX_TPICK_BINS>(p.bins, lds32, [&](u32 b, u32 before, u32) { p.cursor[b] = before; });
        if (threadIdx.x == 0) p.nscan[0] = over ? 0u : all;
    }
}

template <class P>
__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_class_apply_k(const typename P::In t, const RcxClassPlan p, u64* kept)
{
    constexpr u32 KEYS = P::KEYS;
    constexpr u64 LOW = (1ull << RCX_TPICK_COUNT_SHIFT) - 1ull;
    __shared__ u64 lds[KEYS][4];
    const u64 count = rcx_pick_count(t.count, t.max_pick);
    const u64 tiles = rcx_tpick_tiles(P::KEPT ? t.max_pick : count); // (KEPT: every entry's kept is written, also behind the count)
    const bool over = p.nscan[1] != 0u;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        const u32 key = k < count && !over ? p.keys[k] : RCX_TPICK_NONE;
        const bool live = key != RCX_TPICK_NONE;
        const u32 len = live ? (u32)t.len[k] : 0u;
        const u32 w = live ? t.widths[k] : 1u;
        const bool classed = live && key < KEYS;
        const u64 value = classed ? (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units(len, w) : 0ull;
        u64 before, total;
        rcx_class_tile_scan<KEYS>(key, value, lds, before, total);
        bool placed = false;
        if (classed) {
            const u32 c = P::class_of(key);
            const RcxClassSet& s = P::SETS > 1 && P::set_of(key) ? p.set[1] : p.set[0];
            const u64 place = (u64)s.classes->ent_first[c] + p.tile_ents[tile * KEYS + key] + (before >> RCX_TPICK_COUNT_SHIFT);
            if (place < t.max_pick) { // (it is: the classes hold at most `count` entries between them)
                s.ufirst[place] = s.classes->ubase[c] + p.tile_units[tile * KEYS + key] + (before & LOW);
                s.from[place] = t.src_at[k];
                s.to[place] = t.dst_at[k];
                s.len[place] = len;
                if constexpr (P::SETS > 1)
                    if (s.bat) s.bat[place] = t.base_at[k]; // (an entry of such a set passed the checks: base_at is given)
                placed = true;
            }
        }
        if constexpr (P::SCAN) {
            const bool scan = live && key >= KEYS;
            const u32 at = rcx_pick_take(p.cursor, key - KEYS, scan);
            if (scan && (u64)at < t.max_pick) {
                p.scan_from[at] = t.src_at[k];
                p.scan_to[at] = t.dst_at[k];
                p.scan_len[at] = len;
                p.scan_kind[at] = (u8)(w | ((u32)t.preds[k] << 4));
            }
        }
        if constexpr (P::KEPT)
            if (kept && k < t.max_pick) kept[k] = placed ? (u64)len : 0ull;
    }
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_class_rows_k(const RcxClassSet s, u64 rows_most)
{
    const RcxTypedClasses& cl = *s.classes;
    u64 rows = cl.row_first[RCX_TYPED_CLASSES];
    if (rows > rows_most) rows = rows_most; // (it is not: the bytes are at most max_bytes)
    for (u64 r = (u64)blockIdx.x * RCX_TPICK_THREADS + threadIdx.x; r < rows; r += (u64)gridDim.x * RCX_TPICK_THREADS)
        s.rowtab[r] = rcx_class_row(cl, s.ufirst, (u32)r);
}

#endif // !RCX_HOST_SIM
