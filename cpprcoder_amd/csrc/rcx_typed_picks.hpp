// rcx_typed_picks.hpp -- the planner of rcx_typed_join_picks_device (include/rcx_typed_picks.h): what rcx_typed_plan(...,
// scan = true) does on the host (rcx_typed_items.hpp, whose comment block says what the tables must hold) for entries that
// lie in device memory, each with a source and a destination position of its own.  Launches that follow one another:
//
//   rcx_tpick_clear_k     bins[] = 0, by a kernel: a captured call is kernel nodes alone.
//   rcx_tpick_classify_k  entry k < min(*count, max_pick): validate it (rcx_tpick_validate) and give it a KEY: its class
//                         without a predictor (0 .. 3 = width 1, 2, 4, 8), 4 + its length bin with one, or none.  A TILE is
//                         the 256 entries of a workgroup's turn; tile_sum[tile] = per class the entries and their whole
//                         units, and the bytes of all the tile's valid entries.  bins[] counts the scan list's bins, a wave
//                         at a time (rcx_pick_take).
//   rcx_tpick_top_k       one workgroup, 1024 tiles a pass: the exclusive sums over the tiles (tile_ents, tile_units), from
//                         their totals the head of the tables (RcxTypedClasses, as rcx_typed_plan computes it) and
//                         ufirst[nent]; the bytes against max_bytes -- above it the head is all zero, the scan list's length
//                         0 and RCX_E_CAPACITY latched at the count, so the walking kernels find nothing to do; the bins'
//                         cursors.
//   rcx_tpick_apply_k     the tiles again: an entry without a predictor takes place ent_first[class] + tile_ents + its rank
//                         in the tile -- the caller's order within the class, as the host plan has it -- and
//                         ufirst[place] = ubase[class] + tile_units + the units before it in the tile, an exact prefix sum
//                         in the placed order; an entry with one takes the next place of its bin in the scan list.
//   rcx_tpick_rows_k      rowtab: row r of a class = the entry of unit ubase + 256 r, by bisection over the class's entries
//                         (rcx_typed_locate, the kernels' own search), and the class's last entry once more.
//
// Then rcx_typed_picks_items_k and rcx_typed_picks_scan_k (rcx_typed_items.hpp) walk the tables.  No wave waits for another:
// what one launch leaves the next one reads.  The sums are exact (u64 units, u32 entries), the scan list's order is a
// counting sort as rcx_picks.hpp's: exact below 512 bytes, 1 part in 256 above; which place of its bin an entry gets differs
// from call to call and no output depends on it.  Nothing is read behind min(*count, max_pick).
//
// The rules per entry are plain functions, also compiled into tests/sim/typed_picks_san.cpp.
#pragma once

#include "../../include/rcx_predict.h" // RCX_PRED_*, RCX_MAX_BLOCK
#include "rcx_typed_items.hpp"

#define RCX_TPICK_THREADS 256u                                        // entries of a tile = threads of a planner workgroup
#define RCX_TPICK_GRID 512u                                           // workgroups of the planner's entry kernels at the most: they loop
#define RCX_TPICK_TOP 1024u                                           // tiles a pass of the one workgroup over the tile sums
#define RCX_TPICK_EXACT 512u                                          // scan list: lengths below this have a bin each
#define RCX_TPICK_BINS (RCX_TPICK_EXACT + (27u - 9u) * 256u)          // 5120: an entry has less than 2^27 bytes
#define RCX_TPICK_NONE 0xFFFFFFFFu
#define RCX_TPICK_MAX_BYTES (1ull << 42)                              // max_bytes at the most: 2^30 + 8 rows
#define RCX_TPICK_OK 0u
#define RCX_TPICK_CAPACITY 1u // = RCX_ST_CAPACITY
#define RCX_TPICK_CORRUPT 2u  // = RCX_ST_CORRUPT
#define RCX_TPICK_COUNT_SHIFT 40u // a tile's sum of a class: entries << 40 | whole units (below 2^23 an entry, 256 entries)

// ---- the rules per entry: plain functions ----------------------------------------------------------------------------------
// An entry of len > 0 bytes: RCX_TPICK_OK, or what it is skipped with.  No sum that can wrap.
RCX_HD u32 rcx_tpick_validate(u64 src_at, u64 dst_at, u64 len, u32 w, u32 pr, u64 src_cap, u64 dst_cap)
{
    if (!(w == 1 || w == 2 || w == 4 || w == 8) || pr > RCX_PRED_ZIGZAG || (w == 1 && pr != RCX_PRED_NONE)) return RCX_TPICK_CORRUPT;
    if (len / w + len % w > RCX_MAX_BLOCK) return RCX_TPICK_CORRUPT;
    if (src_at > src_cap || len > src_cap - src_at || dst_at > dst_cap || len > dst_cap - dst_at) return RCX_TPICK_CAPACITY;
    return RCX_TPICK_OK;
}

// the bin of a scan entry of `len` bytes, 1 <= len < 2^27: ascending bins = descending length
RCX_HD u32 rcx_tpick_bin(u32 len)
{
    u32 up = len;
    if (len >= RCX_TPICK_EXACT) {
        u32 e = 9;
        while ((len >> e) > 1u) ++e; // the leading one, 9 .. 26
        up = RCX_TPICK_EXACT + (e - 9u) * 256u + ((len >> (e - 8u)) & 255u);
    }
    return RCX_TPICK_BINS - 1u - up;
}

// the key of a valid entry: 0 .. 3 = the class 3 * key of rcx_typed_class without a predictor, 4 + bin = the scan list
RCX_HD u32 rcx_tpick_key(u32 len, u32 w, u32 pr) { return pr ? 4u + rcx_tpick_bin(len) : (w == 1 ? 0u : w == 2 ? 1u : w == 4 ? 2u : 3u); }
RCX_HD u64 rcx_tpick_units(u32 len, u32 w) { return (u64)((len / w) >> 4); }

// rows of rowtab at the most when the valid entries have max_bytes between them: a unit has 16 bytes at least, a row 256 units,
// every class one more row than whole ones and one closing entry
RCX_HD u64 rcx_tpick_rows_most(u64 max_bytes) { return max_bytes / (16u * RCX_TYPED_ROW) + 8u; }
RCX_HD u64 rcx_tpick_tiles(u64 entries) { return (entries + RCX_TPICK_THREADS - 1) / RCX_TPICK_THREADS; }

// The head of the tables from the four classes' entries and whole units (classes 0, 3, 6, 9 of rcx_typed_class): what
// rcx_typed_plan computes.
RCX_HD void rcx_tpick_head(const u64* nent4, const u64* units4, RcxTypedClasses& cl)
{
    u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c) {
        const u32 w = rcx_typed_class_width(c);
        const u64 n = c % 3u ? 0 : nent4[c / 3u], un = c % 3u ? 0 : units4[c / 3u];
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

// Row r of rowtab (r below row_first[RCX_TYPED_CLASSES]): the entry of the row's first unit, or the class's last entry for
// the row that closes the class.
RCX_DEV u32 rcx_tpick_row(const RcxTypedClasses& cl, const u64* ufirst, u32 r)
{
    u32 c = 0;
    while (r >= cl.row_first[c + 1]) ++c;
    const u32 local = r - cl.row_first[c], nrow = cl.row_first[c + 1] - cl.row_first[c] - 1u;
    const u32 first = cl.ent_first[c], last = cl.ent_first[c + 1] - 1u;
    if (local == nrow) return last;
    return rcx_typed_locate(ufirst, first, last, cl.ubase[c] + (u64)local * RCX_TYPED_ROW);
}

#if !defined(RCX_HOST_SIM)

#include "rcx_picks.hpp" // rcx_pick_take

static_assert(RCX_TPICK_CAPACITY == RCX_ST_CAPACITY && RCX_TPICK_CORRUPT == RCX_ST_CORRUPT, "the rules return the latch's flags");

// What the call is given, as the kernels take it.
struct RcxTypedPickIn {
    const u64* src_at;
    const u64* dst_at;
    const u64* len;
    const u8* widths;
    const u8* preds; // or nullptr
    const u64* count;
    u64 max_pick, max_bytes, src_cap, dst_cap;
};

// The planned tables and the planner's own words, all in the context's table scratch (rcx_typed_picks_api.hpp has the layout).
struct RcxTypedPickPlan {
    RcxTypedClasses* classes;
    u64* ufirst;     // [max_pick + 1]
    u64* from;       // [max_pick]
    u64* to;         // [max_pick]
    u64* scan_from;  // [max_pick]
    u64* scan_to;    // [max_pick]
    u64* tile_sum;   // [tiles][5]: classes 0 .. 3 (entries << 40 | units), bytes
    u64* tile_units; // [tiles][4]: the units of the class in the tiles before
    u32* tile_ents;  // [tiles][4]: the entries, likewise
    u32* len;        // [max_pick]
    u32* scan_len;   // [max_pick]
    u32* keys;       // [max_pick]
    u32* rowtab;     // [rcx_tpick_rows_most(max_bytes)]
    u32* cursor;     // [RCX_TPICK_BINS]
    u32* bins;       // [RCX_TPICK_BINS], zero when the classify kernel starts
    u32* nscan;      // [2]: the scan list's length; 1 if the bytes were above max_bytes
    u8* scan_kind;   // [max_pick]
};

__device__ __forceinline__ u64 rcx_tpick_count(const RcxTypedPickIn& t)
{
    const u64 c = t.count[0];
    return c < t.max_pick ? c : t.max_pick;
}

// A tile's sums: every thread of the workgroup gives its key (a class 0 .. 3, or anything else: no class) and its value
// (1 << 40 | units).  before = what the threads below it gave to ITS class, total[c] = what the tile gave to class c.
// lds: 4 x 4 words; ends with the workgroup in step, so that lds may be used again.
__device__ __forceinline__ void rcx_tpick_tile_scan(u32 key, u64 value, u64 (*lds)[4], u64& before, u64 (&total)[4])
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 upto[4];
#pragma unroll
    for (u32 c = 0; c < 4; ++c) {
        upto[c] = rcx_wave_scan<u64>(key == c ? value : 0ull, lane);
        if (lane == 63u) lds[c][wave] = upto[c];
    }
    __syncthreads();
    before = 0;
#pragma unroll
    for (u32 c = 0; c < 4; ++c) {
        u64 front = 0, all = 0;
#pragma unroll
        for (u32 w = 0; w < 4; ++w) {
            const u64 x = lds[c][w];
            front += w < wave ? x : 0ull;
            all += x;
        }
        total[c] = all;
        if (key == c) before = front + upto[c] - value;
    }
    __syncthreads();
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_tpick_clear_k(const RcxTypedPickPlan p)
{
    const u32 b = blockIdx.x * RCX_TPICK_THREADS + threadIdx.x;
    if (b < RCX_TPICK_BINS) p.bins[b] = 0;
    if (b < 2u) p.nscan[b] = 0;
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_tpick_classify_k(const RcxTypedPickIn t, const RcxTypedPickPlan p, u32* status)
{
    __shared__ u64 lds[4][4];
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
                    key = rcx_tpick_key((u32)len, w, pr);
                    value = (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units((u32)len, w);
                    bytes = len;
                }
            }
            p.keys[k] = key;
        }
        const bool scan = key != RCX_TPICK_NONE && key >= 4u;
        (void)rcx_pick_take(p.bins, key - 4u, scan);
        // the bytes of the tile
        u64 sum = bytes;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((threadIdx.x & 63u) == 0) wave_bytes[threadIdx.x >> 6] = sum;
        u64 before, total[4];
        rcx_tpick_tile_scan(key, value, lds, before, total); // (in step twice: wave_bytes is read behind the first)
        if (threadIdx.x < 4u) p.tile_sum[tile * 5u + threadIdx.x] = total[threadIdx.x];
        if (threadIdx.x == 4u) p.tile_sum[tile * 5u + 4u] = wave_bytes[0] + wave_bytes[1] + wave_bytes[2] + wave_bytes[3];
        __syncthreads(); // (wave_bytes is written again in the next turn)
    }
}

// Inclusive sums over the 1024 threads of the one workgroup; all = the workgroup's total.  lds: 16 words; in step at its end.
template <class T>
__device__ __forceinline__ T rcx_tpick_top_scan(T x, T* lds, T& all)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T upto = rcx_wave_scan<T>(x, lane);
    if (lane == 63u) lds[wave] = upto;
    __syncthreads();
    T front = 0;
    all = 0;
#pragma unroll
    for (u32 w = 0; w < RCX_TPICK_TOP / 64u; ++w) {
        const T v = lds[w];
        front += w < wave ? v : (T)0;
        all += v;
    }
    __syncthreads();
    return upto + front;
}

__global__ __launch_bounds__(RCX_TPICK_TOP) void rcx_tpick_top_k(const RcxTypedPickIn t, const RcxTypedPickPlan p, u32* status)
{
    __shared__ u64 lds[RCX_TPICK_TOP / 64u];
    __shared__ u32 lds32[RCX_TPICK_TOP / 64u];
    __shared__ u64 totals[8]; // the four classes' entries and units, for the one thread that writes the head
    const u64 count = rcx_tpick_count(t), tiles = rcx_tpick_tiles(count);
    u64 ents[4] = {}, units[4] = {}, bytes = 0; // of the tiles before this pass (the same in every thread)
    for (u64 base = 0; base < tiles; base += RCX_TPICK_TOP) {
        const u64 tile = base + threadIdx.x;
        const bool has = tile < tiles;
#pragma unroll
        for (u32 c = 0; c < 4; ++c) {
            const u64 v = has ? p.tile_sum[tile * 5u + c] : 0ull;
            const u64 n = v >> RCX_TPICK_COUNT_SHIFT, un = v & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull);
            u64 all_n, all_un;
            const u64 upto_n = rcx_tpick_top_scan<u64>(n, lds, all_n), upto_un = rcx_tpick_top_scan<u64>(un, lds, all_un);
            if (has) {
                p.tile_ents[tile * 4u + c] = (u32)(ents[c] + upto_n - n);
                p.tile_units[tile * 4u + c] = units[c] + upto_un - un;
            }
            ents[c] += all_n;
            units[c] += all_un;
        }
        u64 all_bytes;
        (void)rcx_tpick_top_scan<u64>(has ? p.tile_sum[tile * 5u + 4u] : 0ull, lds, all_bytes);
        bytes += all_bytes;
    }
    const bool over = bytes > t.max_bytes;
    if (threadIdx.x == 0) {
        if (over) rcx_flag(status, RCX_ST_CAPACITY, count);
#pragma unroll
        for (u32 c = 0; c < 4; ++c) {
            totals[c] = over ? 0ull : ents[c];
            totals[4 + c] = over ? 0ull : units[c];
        }
        RcxTypedClasses& cl = *p.classes;
        rcx_tpick_head(totals, totals + 4, cl);
        p.ufirst[cl.ent_first[RCX_TYPED_CLASSES]] = cl.ubase[RCX_TYPED_CLASSES];
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

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_tpick_apply_k(const RcxTypedPickIn t, const RcxTypedPickPlan p)
{
    __shared__ u64 lds[4][4];
    const u64 count = rcx_tpick_count(t), tiles = rcx_tpick_tiles(count);
    const RcxTypedClasses* const cl = p.classes;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 k = tile * RCX_TPICK_THREADS + threadIdx.x;
        const u32 key = k < count ? p.keys[k] : RCX_TPICK_NONE;
        const bool live = key != RCX_TPICK_NONE;
        const u32 len = live ? (u32)t.len[k] : 0u;
        const u32 w = live ? t.widths[k] : 1u;
        const u64 value = live && key < 4u ? (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units(len, w) : 0ull;
        u64 before, total[4];
        rcx_tpick_tile_scan(key, value, lds, before, total);
        if (live && key < 4u) {
            const u32 c = 3u * key;
            const u64 place = (u64)cl->ent_first[c] + p.tile_ents[tile * 4u + key] + (before >> RCX_TPICK_COUNT_SHIFT);
            if (place < t.max_pick) { // (it is: the classes hold at most `count` entries between them)
                p.ufirst[place] = cl->ubase[c] + p.tile_units[tile * 4u + key] + (before & ((1ull << RCX_TPICK_COUNT_SHIFT) - 1ull));
                p.from[place] = t.src_at[k];
                p.to[place] = t.dst_at[k];
                p.len[place] = len;
            }
        }
        const bool scan = live && key >= 4u;
        const u32 s = rcx_pick_take(p.cursor, key - 4u, scan);
        if (scan && (u64)s < t.max_pick) {
            p.scan_from[s] = t.src_at[k];
            p.scan_to[s] = t.dst_at[k];
            p.scan_len[s] = len;
            p.scan_kind[s] = (u8)(w | ((u32)t.preds[k] << 4));
        }
    }
}

__global__ __launch_bounds__(RCX_TPICK_THREADS) void rcx_tpick_rows_k(const RcxTypedPickPlan p, u64 rows_most)
{
    const RcxTypedClasses& cl = *p.classes;
    u64 rows = cl.row_first[RCX_TYPED_CLASSES];
    if (rows > rows_most) rows = rows_most; // (it is not: the bytes are at most max_bytes)
    for (u64 r = (u64)blockIdx.x * RCX_TPICK_THREADS + threadIdx.x; r < rows; r += (u64)gridDim.x * RCX_TPICK_THREADS)
        p.rowtab[r] = rcx_tpick_row(cl, p.ufirst, (u32)r);
}

#endif // !RCX_HOST_SIM
