// rcx_base_picks.hpp -- the planner of rcx_base_join_picks_device (include/rcx_base_picks.h): what rcx_base_items_plan(...,
// scan = true) does on the host (rcx_base_items.hpp) for entries that lie in device memory, each with a source, a base and a
// destination position of its own; and the kernel that walks the base set it leaves.  The plan has the host plan's two sets:
//   the typed set   the entries WITHOUT an op: 4 classes by width and the scan list for those with a predictor -- the tables
//                   rcx_typed_picks.hpp's planner makes when the entries with an op are left out, word for word
//   the base set    the entries WITH an op: 12 classes, 3 * log2(width) + op, a workgroup step of RCX_BASE_ROWS(width) rows,
//                   ufirst, from, to, len, rowtab and bat[k] = the entry's offset in the base
//
// ONE planner for both sets, with 16 class keys: key 0 .. 3 = the typed classes, 4 .. 15 = 4 + the base class, 16 + bin = the
// scan list.  A second instance of rcx_typed_picks.hpp's kernels per set would read every entry twice and validate it twice,
// and its classify kernel cannot know an op; one classify kernel with 16 sums a tile reads an entry once, and the 16 scans
// are registers and cross-lane moves, which the planner has to spare: it is bound by its table reads.  Launches that follow one
// another:
//
//   rcx_tpick_clear_k     (rcx_typed_picks.hpp, as it is) bins[] = 0
//   rcx_bpick_classify_k  entry k < min(*count, max_pick): validate it (rcx_bpick_validate), give it its key; per tile of 256
//                         entries the 16 classes' entries and whole units, and the bytes of all its valid entries; bins[]
//   rcx_bpick_top_k       one workgroup: the exclusive sums over the tiles for the 16 classes, both heads (rcx_tpick_head,
//                         rcx_bpick_head) and both closing ufirst; the bytes against max_bytes -- above it both heads are
//                         zero, the scan list empty and RCX_E_CAPACITY latched at the count; the bins' cursors
//   rcx_bpick_apply_k     the tiles again: every entry takes its place in its class of its set, the caller's order within the
//                         class kept, ufirst an exact prefix sum; or the next place of its bin in the scan list
//   rcx_tpick_rows_k      (as it is) twice: the typed set's row table, then the base set's -- the row rule (rcx_tpick_row)
//                         reads only a head and a ufirst and is the same for both
//
// Then rcx_typed_picks_items_k and rcx_typed_picks_scan_k (rcx_typed_items.hpp, as they are) walk the typed set and
// rcx_base_picks_items_k, below, the base set.  No wave waits for another; nothing is read behind min(*count, max_pick).
//
// The rules per entry are plain functions, also compiled into tests/sim/base_picks_san.cpp.
#pragma once

#include "../../include/rcx_base.h" // RCX_BASE_SUBZZ
#include "rcx_base_items.hpp"
#include "rcx_typed_picks.hpp"

#define RCX_BPICK_TYPED 4u                      // keys 0 .. 3: the typed set's classes without a predictor, by width
#define RCX_BPICK_KEYS 16u                      // keys 4 .. 15: 4 + the base set's class; 16 + bin: the scan list
#define RCX_BPICK_SUMS (RCX_BPICK_KEYS + 1u)    // a tile's sums: the 16 keys, then the bytes

// ---- the rules per entry: plain functions ----------------------------------------------------------------------------------
// An entry of len > 0 bytes: RCX_TPICK_OK, or what it is skipped with: everything corrupt before anything of capacity.  op =
// RCX_BASE_NONE_OP: rcx_tpick_validate's answer, and base_at is not looked at.  No sum that can wrap.
RCX_HD u32 rcx_bpick_validate(u64 src_at, u64 dst_at, u64 base_at, u64 len, u32 w, u32 pr, u32 op, u64 src_cap, u64 dst_cap, u64 base_cap)
{
    const u32 bad = rcx_tpick_validate(src_at, dst_at, len, w, pr, src_cap, dst_cap);
    if (bad == RCX_TPICK_CORRUPT) return bad;
    if (op != RCX_BASE_NONE_OP && (op > RCX_BASE_SUBZZ || pr != RCX_PRED_NONE)) return RCX_TPICK_CORRUPT;
    if (bad) return bad;
    if (op != RCX_BASE_NONE_OP && (base_at > base_cap || len > base_cap - base_at)) return RCX_TPICK_CAPACITY;
    return RCX_TPICK_OK;
}

// the key of a valid entry
RCX_HD u32 rcx_bpick_key(u32 len, u32 w, u32 pr, u32 op)
{
    if (op != RCX_BASE_NONE_OP) return RCX_BPICK_TYPED + rcx_typed_class(w, op);
    return pr ? RCX_BPICK_KEYS + rcx_tpick_bin(len) : rcx_tpick_key(len, w, 0u);
}

// rows of the base set's rowtab at the most when the valid entries have max_bytes between them: a unit has 16 bytes at least, a
// row 256 units, and each of the 12 classes one more row than whole ones and one closing entry: max_bytes / 4096 + 24
RCX_HD u64 rcx_bpick_rows_most(u64 max_bytes) { return max_bytes / (16u * RCX_TYPED_ROW) + 2u * RCX_TYPED_CLASSES; }

// The head of the base set from its 12 classes' entries and whole units: what rcx_base_items_plan computes for set 1.
RCX_HD void rcx_bpick_head(const u64* nent12, const u64* units12, RcxTypedClasses& cl)
{
    u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c) {
        const u32 w = rcx_typed_class_width(c);
        const u64 n = nent12[c], un = units12[c];
        cl.ent_first[c] = (u32)ents;
        cl.row_first[c] = (u32)rows;
        cl.ubase[c] = ub;
        const u64 step = (u64)rcx_base_items_rows(1u, w) * RCX_TYPED_ROW;
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

// What the call is given, as the kernels take it.
struct RcxBasePickIn {
    const u64* src_at;
    const u64* base_at; // or nullptr: no entry with an op can be valid (base_cap is 0), or none has an op
    const u64* dst_at;
    const u64* len;
    const u8* widths;
    const u8* preds; // or nullptr
    const u8* ops;   // or nullptr
    const u64* count;
    u64 max_pick, max_bytes, src_cap, base_cap, dst_cap;
};

// The planned tables and the planner's own words, all in the context's table scratch (rcx_base_picks_api.hpp has the layout).
struct RcxBasePickPlan {
    RcxTypedClasses* classes;  // the typed set's head
    RcxTypedClasses* bclasses; // the base set's
    u64* ufirst;     // [max_pick + 1] typed set
    u64* bufirst;    // [max_pick + 1] base set
    u64* from;       // [max_pick] typed set
    u64* to;
    u64* bfrom;      // [max_pick] base set
    u64* bto;
    u64* bat;
    u64* scan_from;  // [max_pick]
    u64* scan_to;
    u64* tile_sum;   // [tiles][17]: keys 0 .. 15 (entries << 40 | units), bytes
    u64* tile_units; // [tiles][16]: the units of the key in the tiles before
    u32* tile_ents;  // [tiles][16]: the entries, likewise
    u32* len;        // [max_pick] typed set
    u32* blen;       // [max_pick] base set
    u32* scan_len;   // [max_pick]
    u32* keys;       // [max_pick]
    u32* rowtab;     // [rcx_tpick_rows_most(max_bytes)]
    u32* browtab;    // [rcx_bpick_rows_most(max_bytes)]
    u32* cursor;     // [RCX_TPICK_BINS]
    u32* bins;       // [RCX_TPICK_BINS], zero when the classify kernel starts
    u32* nscan;      // [2]
    u8* scan_kind;   // [max_pick]
};

__device__ __forceinline__ u64 rcx_bpick_count(const RcxBasePickIn& t)
{
    const u64 c = t.count[0];
    return c < t.max_pick ? c : t.max_pick;
}

// rcx_tpick_tile_scan for 16 keys.  lds: 16 x 4 words; ends with the workgroup in step.
__device__ __forceinline__ void rcx_bpick_tile_scan(u32 key, u64 value, u64 (*lds)[4], u64& before, u64& total_mine)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 mine = 0; // the inclusive sum of the thread's own key in its wave
#pragma unroll
    for (u32 c = 0; c < RCX_BPICK_KEYS; ++c) {
        const u64 upto = rcx_wave_scan<u64>(key == c ? value : 0ull, lane);
        if (lane == 63u) lds[c][wave] = upto;
        if (key == c) mine = upto;
    }
    __syncthreads();
    before = 0;
    // total_mine: thread c < 16 gets the tile's total of key c
    const u32 c_total = threadIdx.x < RCX_BPICK_KEYS ? threadIdx.x : 0u;
    total_mine = lds[c_total][0] + lds[c_total][1] + lds[c_total][2] + lds[c_total][3];
    if (key < RCX_BPICK_KEYS) {
        u64 front = 0;
#pragma unroll
        for (u32 w = 0; w < 4; ++w) front += w < wave ? lds[key][w] : 0ull;
        before = front + mine - value;
    }
    __syncthreads();
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_bpick_classify_k(const RcxBasePickIn t, const RcxBasePickPlan p, u32* status)
{
    __shared__ u64 lds[RCX_BPICK_KEYS][4];
    __shared__ u64 wave_bytes[4];
    const u64 count = rcx_bpick_count(t);
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.count[0] > t.max_pick) rcx_flag(status, RCX_ST_CAPACITY, t.max_pick);
    const u64 tiles = rcx_tpick_tiles(count);
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (whole workgroups go round)
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        u32 key = RCX_TPICK_NONE;
        u64 value = 0, bytes = 0;
        if (k < count) {
            const u64 len = t.len[k];
            if (len != 0) { // (a length of 0 is not looked at)
                const u32 w = t.widths[k], pr = t.preds ? t.preds[k] : 0u, op = t.ops ? t.ops[k] : RCX_BASE_NONE_OP;
                const u64 base_at = op != RCX_BASE_NONE_OP && t.base_at ? t.base_at[k] : 0ull; // (not read for an entry without an op)
                const u32 bad = rcx_bpick_validate(t.src_at[k], t.dst_at[k], base_at, len, w, pr, op, t.src_cap, t.dst_cap, t.base_cap);
                if (bad) {
                    rcx_flag(status, bad, k);
                } else {
                    key = rcx_bpick_key((u32)len, w, pr, op);
                    value = (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units((u32)len, w);
                    bytes = len;
                }
            }
            p.keys[k] = key;
        }
        const bool scan = key != RCX_TPICK_NONE && key >= RCX_BPICK_KEYS;
        (void)rcx_pick_take(p.bins, key - RCX_BPICK_KEYS, scan);
        u64 sum = bytes;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((threadIdx.x & 63u) == 0) wave_bytes[threadIdx.x >> 6] = sum;
        u64 before, total;
        rcx_bpick_tile_scan(key, value, lds, before, total); // (in step twice: wave_bytes is read behind the first)
        if (threadIdx.x < RCX_BPICK_KEYS) p.tile_sum[tile * RCX_BPICK_SUMS + threadIdx.x] = total;
        if (threadIdx.x == RCX_BPICK_KEYS) p.tile_sum[tile * RCX_BPICK_SUMS + RCX_BPICK_KEYS] = wave_bytes[0] + wave_bytes[1] + wave_bytes[2] + wave_bytes[3];
        __syncthreads(); // (wave_bytes is written again in the next turn)
    }
}

__global__ __launch_bounds__(RCX_TPICK_TOP) void rcx_bpick_top_k(const RcxBasePickIn t, const RcxBasePickPlan p, u32* status)
{
    __shared__ u64 lds[RCX_TPICK_TOP / 64u];
    __shared__ u32 lds32[RCX_TPICK_TOP / 64u];
    __shared__ u64 totals[2 * RCX_BPICK_KEYS]; // the 16 keys' entries, then their units, for the one thread that writes the heads
    const u64 count = rcx_bpick_count(t), tiles = rcx_tpick_tiles(count);
    u64 bytes = 0;
    for (u32 c = 0; c < RCX_BPICK_KEYS; ++c) { // (a loop, not unrolled: one key's sums over all tiles at a time)
        u64 ents = 0, units = 0; // of the tiles before this pass (the same in every thread)
        for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
            const u64 tile = base + threadIdx.x;
            const bool has = tile < tiles;
            const u64 v = has ? p.tile_sum[tile * RCX_BPICK_SUMS + c] : 0ull;
            const u64 n = v >> RCX_TPICK_COUNT_SHIFT, un = v & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull);
            u64 all_n, all_un;
            const u64 upto_n = rcx_tpick_top_scan<u64>(n, lds, all_n), upto_un = rcx_tpick_top_scan<u64>(un, lds, all_un);
            if (has) {
                p.tile_ents[tile * RCX_BPICK_KEYS + c] = (u32)(ents + upto_n - n);
                p.tile_units[tile * RCX_BPICK_KEYS + c] = units + upto_un - un;
            }
            ents += all_n;
            units += all_un;
        }
        if (threadIdx.x == 0) {
            totals[c] = ents;
            totals[RCX_BPICK_KEYS + c] = units;
        }
    }
    for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
        const u64 tile = base + threadIdx.x;
        u64 all_bytes;
        (void)rcx_tpick_top_scan<u64>(tile < tiles ? p.tile_sum[tile * RCX_BPICK_SUMS + RCX_BPICK_KEYS] : 0ull, lds, all_bytes);
        bytes += all_bytes;
    }
    const bool over = bytes > t.max_bytes;
    if (threadIdx.x == 0) { // (totals[] is this thread's own writing)
        if (over) {
            rcx_flag(status, RCX_ST_CAPACITY, count);
            for (u32 c = 0; c < 2 * RCX_BPICK_KEYS; ++c) totals[c] = 0;
        }
        RcxTypedClasses& cl = *p.classes;
        rcx_tpick_head(totals, totals + RCX_BPICK_KEYS, cl);
        p.ufirst[cl.ent_first[RCX_TYPED_CLASSES]] = cl.ubase[RCX_TYPED_CLASSES];
        RcxTypedClasses& bcl = *p.bclasses;
        rcx_bpick_head(totals + RCX_BPICK_TYPED, totals + RCX_BPICK_KEYS + RCX_BPICK_TYPED, bcl);
        p.bufirst[bcl.ent_first[RCX_TYPED_CLASSES]] = bcl.ubase[RCX_TYPED_CLASSES];
        p.nscan[1] = over ? 1u : 0u;
    }
    // the scan list: cursor[b] = the entries of the bins before b
    constexpr u32 PER = (RCX_TPICK_BINS + RCX_TPICK_TOP - 1) / RCX_TPICK_TOP;
    const u32 b0 = threadIdx.x * PER;
    u32 mine[PER], sum = 0;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        mine[j] = b0 + j < RCX_TPICK_BINS ? p.bins[b0 + j] : 0u;
        sum += mine[j];
    }
    u32 all;
    u32 before = rcx_tpick_top_scan<u32>(sum, lds32, all) - sum;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (b0 + j < RCX_TPICK_BINS) p.cursor[b0 + j] = before;
        before += mine[j];
    }
    if (threadIdx.x == 0) p.nscan[0] = over ? 0u : all;
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_bpick_apply_k(const RcxBasePickIn t, const RcxBasePickPlan p)
{
    __shared__ u64 lds[RCX_BPICK_KEYS][4];
    const u64 count = rcx_bpick_count(t), tiles = rcx_tpick_tiles(count);
    const RcxTypedClasses* const cl = p.classes;
    const RcxTypedClasses* const bcl = p.bclasses;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        const u32 key = k < count ? p.keys[k] : RCX_TPICK_NONE;
        const bool live = key != RCX_TPICK_NONE;
        const u32 len = live ? (u32)t.len[k] : 0u;
        const u32 w = live ? t.widths[k] : 1u;
        const bool placed = live && key < RCX_BPICK_KEYS;
        const u64 value = placed ? (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units(len, w) : 0ull;
        u64 before, total;
        rcx_bpick_tile_scan(key, value, lds, before, total);
        if (placed) {
            const u64 rank = p.tile_ents[tile * RCX_BPICK_KEYS + key] + (before >> RCX_TPICK_COUNT_SHIFT);
            const u64 unit = p.tile_units[tile * RCX_BPICK_KEYS + key] + (before & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull));
            if (key < RCX_BPICK_TYPED) {
                const u32 c = 3u * key;
                const u64 place = (u64)cl->ent_first[c] + rank;
                if (place < t.max_pick) { // (it is: the classes hold at most `count` entries between them)
                    p.ufirst[place] = cl->ubase[c] + unit;
                    p.from[place] = t.src_at[k];
                    p.to[place] = t.dst_at[k];
                    p.len[place] = len;
                }
            } else {
                const u32 c = key - RCX_BPICK_TYPED;
                const u64 place = (u64)bcl->ent_first[c] + rank;
                if (place < t.max_pick) {
                    p.bufirst[place] = bcl->ubase[c] + unit;
                    p.bfrom[place] = t.src_at[k];
                    p.bto[place] = t.dst_at[k];
                    p.bat[place] = t.base_at[k]; // (an entry with an op passed the checks: base_at is given)
                    p.blen[place] = len;
                }
            }
        }
        const bool scan = live && key >= RCX_BPICK_KEYS;
        const u32 s = rcx_pick_take(p.cursor, key - RCX_BPICK_KEYS, scan);
        if (scan && (u64)s < t.max_pick) {
            p.scan_from[s] = t.src_at[k];
            p.scan_to[s] = t.dst_at[k];
            p.scan_len[s] = len;
            p.scan_kind[s] = (u8)(w | ((u32)t.preds[k] << 4));
        }
    }
}

// ===========================================================================
// The join of the entries with an op over the tables the device planned: rcx_base_items_k<true>'s walk with the loops
// written out again (as rcx_typed_picks_items_k repeats rcx_typed_items_k's: a shared body changed the older kernel's
// code), rcx_base_items_step and rcx_base_items_rest with RcxBasePickTables.  A base set that is empty has a head of zeros
// and the kernel finds no step and no block.
// ===========================================================================
__global__ __launch_bounds__(RCX_BASE_THREADS) void rcx_base_picks_items_k(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst,
                                                                           RcxBasePickTables bt)
{
    constexpr bool JOIN = true;
    const RcxTypedClasses* const cl = bt.classes;
    const u32 tid = threadIdx.x;
    const u64 steps = cl->step_end[RCX_TYPED_CLASSES - 1];
    for (u64 s = blockIdx.x; s < steps; s += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->step_end, s);
        const u64 local = s - (c ? cl->step_end[c - 1] : 0);
        const u64 ubase = cl->ubase[c], total = cl->ubase[c + 1] - ubase;
        const u32 rows = cl->row_first[c];
        rcx_base_items_dispatch(c, [&](auto w_, auto op_) {
            constexpr u32 W = decltype(w_)::value, OP = decltype(op_)::value, K = RCX_BASE_ROWS(W), STEP = K * RCX_TYPED_ROW;
            const u64 base = local * STEP;
            const u32 row0 = rows + (u32)(local * K);
            if (base + STEP <= total) rcx_base_items_step<W, JOIN, OP, false>(src, ref, dst, bt, ubase, base, total, row0, tid);
            else rcx_base_items_step<W, JOIN, OP, true>(src, ref, dst, bt, ubase, base, total, row0, tid);
        });
    }
    const u64 blocks = cl->rest_end[RCX_TYPED_CLASSES - 1];
    for (u64 b = blockIdx.x; b < blocks; b += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->rest_end, b);
        const u64 r = (b - (c ? cl->rest_end[c - 1] : 0)) * RCX_TYPED_ROW + tid;
        const u32 first = cl->ent_first[c], count = cl->ent_first[c + 1] - first;
        rcx_base_items_dispatch(c, [&](auto w_, auto op_) {
            rcx_base_items_rest<decltype(w_)::value, JOIN, decltype(op_)::value>(src, ref, dst, bt, first, count, r);
        });
    }
}

#endif // !RCX_HOST_SIM
