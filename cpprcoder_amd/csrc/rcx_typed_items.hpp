// rcx_typed_items.hpp -- the typed stage per item (include/rcx_typed_items.h): many buffers of differing sizes in one call,
// each with its own element width (1, 2, 4, 8) and predictor (none, delta, zigzag), each transformed as ONE superblock of
// rcx_planes.hpp / rcx_predict.hpp with m = len / w elements: the predictor starts at 0 in front of the item's first
// element, plane p goes to [p * m, (p + 1) * m) of the item's span, the len % w tail bytes keep their places.  Width 1 is a
// copy.  The unit transposes, the predictor's arithmetic, the scan's tile and the byte-addressed accesses are those two
// files'; here is what is new: the plan, the mapping from work to (item, unit), and the two kernels that walk it.
//
// THE PLAN (host, rcx_typed_plan; plain C++, also compiled into tests/sim/typed_items_san.cpp).  An item with bytes gets an
// ENTRY {at, len} in the tables, in the caller's order WITHIN ITS CLASS: class = (width, predictor), 12 at the most.  A
// class is the unit of everything that follows, and that is how the width stays uniform: no wave, no workgroup step and
// no row ever holds entries of two classes, so the kernels branch on the class once a step, on a scalar, and inside the
// branch width and predictor are template arguments.  No lane ever tests a width.
//   units   the whole units (16 elements) of a class's entries, numbered through: ufirst[k] = the first unit of entry k
//           (one array for all classes, ascending; ufirst[nent] closes it), so unit g lies in the LAST entry k with
//           ufirst[k] <= g -- entries without a whole unit share their successor's number and are never found
//   rows    256 consecutive units of a class.  rowtab[row] = the entry of the row's first unit, and one more per class (its
//           last entry), so a lane searches [rowtab[row], rowtab[row + 1]] only: no step when the row lies in one entry (a
//           large item), at most 8 when 256 small ones share it (rcx_typed_locate_step)
//   steps   a workgroup takes RCX_PLANES_U4 / w rows at a time (16 for width 1), all of one class: 16 16-byte registers a
//           lane in flight before the first transpose, as rcx_planes_step does.  The classes' steps are numbered through
//           (step_end), a fixed grid loops over them
//   rests   what is not a whole unit -- the last m % 16 elements and the tail, below 17 * w bytes an entry -- goes byte by
//           byte: entry e of a class owns lanes [e * 17w, (e + 1) * 17w) of the class's rest lanes (rcx_typed_rest_of),
//           in blocks of 256 lanes numbered through like the steps (rest_end)
//   scan    join with a predictor is a prefix sum per item: those entries go to a list of their own, longest first, and
//           rcx_typed_items_scan_k gives a wave whole items as rcx_predict_join_k gives it whole superblocks; width and
//           predictor are read once an item, made scalar, and branched on there
// One upload carries all of it.  Split is one launch, join at most two (rows, scan), whatever the item count.
//
// The kernels read exactly the entries' bytes of src and write exactly the same ranges of dst, at any alignment.  No LDS,
// no barrier, no flag, no scratch, no floating point, no inline assembly; no wave waits for another.
#pragma once

#include <algorithm>
#include <type_traits>
#include <vector>

#include "rcx_predict.hpp"

#define RCX_TYPED_ROW 256u     // units of a row = lanes of a workgroup (RCX_PLANES_THREADS)
#define RCX_TYPED_CLASSES 12u  // 4 widths x 3 predictors; class = 3 * log2(width) + predictor (width 1 has predictor 0 only)

// ---- the mapping: plain functions, also compiled for the host ------------------------------------------------------------
struct RcxTypedClasses {                       // the head of the tables
    u64 step_end[RCX_TYPED_CLASSES];           // workgroup steps of the classes up to and including this one
    u64 rest_end[RCX_TYPED_CLASSES];           // blocks of 256 rest lanes, likewise
    u64 ubase[RCX_TYPED_CLASSES + 1];          // the class's first unit: ufirst[ent_first[c]]
    u32 ent_first[RCX_TYPED_CLASSES + 1];      // its first entry
    u32 row_first[RCX_TYPED_CLASSES + 1];      // its first row in rowtab (a class has rows + 1 entries there)
};

struct RcxTypedTables {
    const RcxTypedClasses* classes;
    const u64* ufirst; // [nent + 1]
    const u64* at;     // [nent] byte offset of the entry in src and dst
    const u32* len;    // [nent] its bytes, >= 1
    const u32* rowtab;
    const u64* scan_at; // the scan list, longest first
    const u32* scan_len;
    const u8* scan_kind; // width | predictor << 4
    u64 nscan;
    static constexpr bool PICKS = false; // (no member: the tables a kernel is handed stay as they are)
};

// The same tables as the planner of rcx_typed_picks.hpp leaves them in device memory: an entry is read at from[k] and
// written at to[k], and the scan list's length is a word in memory.  The walking kernels take either kind (TB).
struct RcxTypedPickTables {
    const RcxTypedClasses* classes;
    const u64* ufirst;
    const u64* from; // [nent] byte offset of the entry in src
    const u64* to;   // [nent] ... and in dst
    const u32* len;
    const u32* rowtab;
    const u64* scan_from;
    const u64* scan_to;
    const u32* scan_len;
    const u8* scan_kind;
    const u32* nscan; // one word
    static constexpr bool PICKS = true;
};

RCX_HD u32 rcx_typed_class(u32 width, u32 pred) { return 3u * (width == 1 ? 0u : width == 2 ? 1u : width == 4 ? 2u : 3u) + pred; }
RCX_HD u32 rcx_typed_class_width(u32 c) { return 1u << (c / 3u); }

// the class of step (or rest block) s: the first whose end lies behind it; s is below end[RCX_TYPED_CLASSES - 1]
RCX_DEV u32 rcx_typed_class_of(const u64* end, u64 s)
{
    u32 c = 0;
    while (s >= end[c]) ++c;
    return c;
}

// One bisection step towards the last k in [lo, hi] with ufirst[k] <= g (ufirst[lo] <= g is given); lo == hi stays as it is.
RCX_DEV void rcx_typed_locate_step(const u64* ufirst, u32& lo, u32& hi, u64 g)
{
    const u32 mid = lo + (hi - lo + 1u) / 2u;
    if (ufirst[mid] <= g) lo = mid;
    else hi = mid - 1u;
}

// the last k in [lo, hi] with ufirst[k] <= g: the entry of unit g (numbered through all classes) of a row whose first unit lies
// in entry lo and whose successor begins in entry hi; the unit is its unit g - ufirst[k].  The kernel takes the same steps for
// the K rows of a workgroup step side by side (rcx_typed_step).
RCX_DEV u32 rcx_typed_locate(const u64* ufirst, u32 lo, u32 hi, u64 g)
{
    while (lo < hi) rcx_typed_locate_step(ufirst, lo, hi, g);
    return lo;
}

// Rest byte j (0 <= j < 17 * W) of an entry of len bytes: 1 = byte p of element e (behind the entry's whole units),
// 2 = the tail byte at e of the entry, 0 = the entry has no such byte.
template <u32 W>
RCX_DEV u32 rcx_typed_rest_of(u32 len, u32 j, u32& e, u32& p)
{
    const u32 m = len / W, e0 = m & ~15u, in_elements = (m - e0) * W;
    if (j < in_elements) {
        e = e0 + j / W;
        p = j % W;
        return 1;
    }
    e = m * W + (j - in_elements);
    p = 0;
    return e < len ? 2u : 0u;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------
struct RcxTypedPlan {
    u64 bytes = 0; // of the tables in `mem`
    u64 o_ufirst = 0, o_at = 0, o_scan_at = 0, o_len = 0, o_rowtab = 0, o_scan_len = 0, o_scan_kind = 0; // byte offsets (the classes lie at 0)
    u64 nent = 0, nrows = 0, nscan = 0, steps = 0, rest_blocks = 0;
};

// keys = (0xFFFFFFFF - len) << 32 | item, len below 2^28, pushed in item order -> ascending: the longest first, equal lengths in
// the caller's order.  Two stable counting passes over 14 bits of the length each where there are many keys (a comparison sort
// was most of the host time of a join call of 200 000 items); the bits above those 28 are the same in every key.
inline void rcx_typed_longest_first(std::vector<u64>& keys)
{
    if (keys.size() < 1024) {
        std::sort(keys.begin(), keys.end());
        return;
    }
    std::vector<u64> other(keys.size());
    std::vector<u32> count(1u << 14);
    for (u32 shift = 32; shift <= 46; shift += 14) {
        std::fill(count.begin(), count.end(), 0u);
        for (const u64 k : keys) count[(k >> shift) & 0x3FFFu] += 1;
        u32 sum = 0;
        for (u32& c : count) {
            const u32 here = c;
            c = sum;
            sum += here;
        }
        for (const u64 k : keys) other[count[(k >> shift) & 0x3FFFu]++] = k;
        keys.swap(other);
    }
}

// Item i = [offs[i], offs[i + 1]) with widths[i] and preds[i] (nullptr = none), all checked before.  scan = true (join): the
// entries with a predictor go to the scan list and get no units, rows or rests.  false if a table outgrows its 32-bit index.
inline bool rcx_typed_plan(const u64* offs, const u8* widths, const u8* preds, u64 nitems, bool scan, std::vector<u64>& mem, RcxTypedPlan& p)
{
    constexpr u32 NC = RCX_TYPED_CLASSES;
    u64 nent[NC] = {}, units[NC] = {};
    std::vector<u64> keys; // the scan list: ascending keys = descending length, then the caller's order
    for (u64 i = 0; i < nitems; ++i) {
        const u64 len = offs[i + 1] - offs[i];
        if (len == 0) continue;
        const u32 w = widths[i], pr = preds ? preds[i] : 0u;
        if (scan && pr) {
            keys.push_back(((u64)(0xFFFFFFFFu - (u32)len) << 32) | i);
            continue;
        }
        const u32 c = rcx_typed_class(w, pr);
        nent[c] += 1;
        units[c] += (len / w) >> 4;
    }
    if (nitems > 0x7FFFFFFFull) return false;
    rcx_typed_longest_first(keys);
    RcxTypedClasses cl{};
    u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
    for (u32 c = 0; c < NC; ++c) {
        const u32 w = rcx_typed_class_width(c);
        cl.ent_first[c] = (u32)ents;
        cl.row_first[c] = (u32)rows;
        cl.ubase[c] = ub;
        const u64 step = (u64)(RCX_PLANES_U4 / w) * RCX_TYPED_ROW;
        steps += (units[c] + step - 1) / step;
        rests += (nent[c] * (17u * w) + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
        cl.step_end[c] = steps;
        cl.rest_end[c] = rests;
        ents += nent[c];
        ub += units[c];
        if (nent[c]) rows += (units[c] + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW + 1;
    }
    if (rows > 0x7FFFFFFFull) return false;
    cl.ent_first[NC] = (u32)ents;
    cl.row_first[NC] = (u32)rows;
    cl.ubase[NC] = ub;
    p.nent = ents;
    p.nrows = rows;
    p.nscan = keys.size();
    p.steps = steps;
    p.rest_blocks = rests;
    // the 8-byte tables first, then the 4-byte ones, then the bytes
    u64 o = (sizeof(RcxTypedClasses) + 7) & ~(u64)7;
    p.o_ufirst = o, o += (ents + 1) * sizeof(u64);
    p.o_at = o, o += ents * sizeof(u64);
    p.o_scan_at = o, o += p.nscan * sizeof(u64);
    p.o_len = o, o += ents * sizeof(u32);
    p.o_rowtab = o, o += rows * sizeof(u32);
    p.o_scan_len = o, o += p.nscan * sizeof(u32);
    p.o_scan_kind = o, o += p.nscan;
    p.bytes = o;
    mem.resize((o + 7) / 8);
    u8* const h = reinterpret_cast<u8*>(mem.data());
    *reinterpret_cast<RcxTypedClasses*>(h) = cl;
    u64* const ufirst = reinterpret_cast<u64*>(h + p.o_ufirst);
    u64* const at = reinterpret_cast<u64*>(h + p.o_at);
    u32* const len = reinterpret_cast<u32*>(h + p.o_len);
    u32* const rowtab = reinterpret_cast<u32*>(h + p.o_rowtab);
    u64 next[NC], unit[NC];
    for (u32 c = 0; c < NC; ++c) next[c] = cl.ent_first[c], unit[c] = cl.ubase[c];
    for (u64 i = 0; i < nitems; ++i) {
        const u64 n = offs[i + 1] - offs[i];
        const u32 w = widths[i], pr = preds ? preds[i] : 0u;
        if (n == 0 || (scan && pr)) continue;
        const u32 c = rcx_typed_class(w, pr);
        const u64 k = next[c]++;
        ufirst[k] = unit[c];
        at[k] = offs[i];
        len[k] = (u32)n;
        unit[c] += (n / w) >> 4;
    }
    ufirst[ents] = ub;
    for (u32 c = 0; c < NC; ++c) {
        if (!nent[c]) continue;
        const u64 nrow = (units[c] + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
        const u32 last = cl.ent_first[c + 1] - 1u;
        u32 k = cl.ent_first[c];
        for (u64 r = 0; r < nrow; ++r) {
            const u64 g = cl.ubase[c] + r * RCX_TYPED_ROW;
            while (k < last && ufirst[k + 1] <= g) ++k;
            rowtab[cl.row_first[c] + r] = k;
        }
        rowtab[cl.row_first[c] + nrow] = last;
    }
    u64* const scan_at = reinterpret_cast<u64*>(h + p.o_scan_at);
    u32* const scan_len = reinterpret_cast<u32*>(h + p.o_scan_len);
    u8* const scan_kind = h + p.o_scan_kind;
    for (u64 s = 0; s < p.nscan; ++s) {
        const u64 i = keys[s] & 0xFFFFFFFFull;
        scan_at[s] = offs[i];
        scan_len[s] = (u32)(offs[i + 1] - offs[i]);
        scan_kind[s] = (u8)(widths[i] | (preds[i] << 4));
    }
    return true;
}

// the tables as a kernel reads them, `base` = where `mem` of rcx_typed_plan lies
inline RcxTypedTables rcx_typed_tables(const u8* base, const RcxTypedPlan& p)
{
    RcxTypedTables t;
    t.classes = reinterpret_cast<const RcxTypedClasses*>(base);
    t.ufirst = reinterpret_cast<const u64*>(base + p.o_ufirst);
    t.at = reinterpret_cast<const u64*>(base + p.o_at);
    t.len = reinterpret_cast<const u32*>(base + p.o_len);
    t.rowtab = reinterpret_cast<const u32*>(base + p.o_rowtab);
    t.scan_at = reinterpret_cast<const u64*>(base + p.o_scan_at);
    t.scan_len = reinterpret_cast<const u32*>(base + p.o_scan_len);
    t.scan_kind = base + p.o_scan_kind;
    t.nscan = p.nscan;
    return t;
}

#if !defined(RCX_HOST_SIM)

// f(width, predictor) as compile-time constants for class c; c is the same in every lane of the workgroup
template <bool JOIN, class F>
__device__ __forceinline__ void rcx_typed_dispatch(u32 c, F f)
{
    typedef std::integral_constant<u32, 0> P0;
    typedef std::integral_constant<u32, 1> P1;
    typedef std::integral_constant<u32, 2> P2;
    typedef std::integral_constant<u32, 1> W1;
    typedef std::integral_constant<u32, 2> W2;
    typedef std::integral_constant<u32, 4> W4;
    typedef std::integral_constant<u32, 8> W8;
    if constexpr (JOIN) { // the classes with a predictor are the scan kernel's
        switch (c) {
        case 0: f(W1{}, P0{}); break;
        case 3: f(W2{}, P0{}); break;
        case 6: f(W4{}, P0{}); break;
        default: f(W8{}, P0{}); break;
        }
    } else {
        switch (c) {
        case 0: f(W1{}, P0{}); break;
        case 3: f(W2{}, P0{}); break;
        case 4: f(W2{}, P1{}); break;
        case 5: f(W2{}, P2{}); break;
        case 6: f(W4{}, P0{}); break;
        case 7: f(W4{}, P1{}); break;
        case 8: f(W4{}, P2{}); break;
        case 9: f(W8{}, P0{}); break;
        case 10: f(W8{}, P1{}); break;
        default: f(W8{}, P2{}); break;
        }
    }
}

// One step of a workgroup in a class of width W: rows row0 .. row0 + K - 1 of rowtab, units base + j * 256 + tid of the class's
// `total`, all loads first.  GUARD = false: every one of them exists; GUARD = true: the class's last step.
template <u32 W, bool JOIN, u32 PRED, bool GUARD, class TB>
__device__ __forceinline__ void rcx_typed_step(const u8* __restrict__ src, u8* __restrict__ dst, const TB& t, u64 ubase, u64 base, u64 total,
                                               u32 row0, u32 tid)
{
    constexpr u32 K = RCX_PLANES_U4 / W;
    u32 w[K][4 * W];
    [[maybe_unused]] typename RcxElem<W>::T prev[K];
    u64 at[K], g[K];
    [[maybe_unused]] u64 out_at[K]; // device-planned tables: where the entry goes, `at` being where it comes from
    u32 m[K], u[K], lo[K], hi[K];
    // Where every row's unit lies, for all K rows before the first load of data, and the K rows' table reads side by side: the
    // memory counter runs down in order, so a table read behind a row's loads would wait for those loads, and a search of
    // one row after the other would put K chains of dependent reads in front of every step.  So: the K rows' bounds; the
    // bisection steps of rcx_typed_locate for all rows at once, as long as any lane of the wave has a row to narrow (none
    // at all where every row lies in one item); the K entries.  A row the class's last step does not have takes the last
    // one it has, and a lane without a unit the class's last unit: both read what is there and use nothing of it.
    const u32 last_row = GUARD ? (u32)((total - 1 - base) / RCX_TYPED_ROW) : K - 1;
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u32 row = row0 + (GUARD && j > last_row ? last_row : j);
        const u64 unit = base + (u64)j * RCX_TYPED_ROW + tid;
        lo[j] = t.rowtab[row];
        hi[j] = t.rowtab[row + 1];
        g[j] = ubase + (GUARD && unit >= total ? total - 1 : unit);
    }
    for (;;) {
        bool more = false;
#pragma unroll
        for (u32 j = 0; j < K; ++j) more |= lo[j] < hi[j];
        if (!__any(more)) break;
#pragma unroll
        for (u32 j = 0; j < K; ++j) rcx_typed_locate_step(t.ufirst, lo[j], hi[j], g[j]);
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        u[j] = (u32)(g[j] - t.ufirst[lo[j]]);
        if constexpr (TB::PICKS) {
            at[j] = t.from[lo[j]];
            out_at[j] = t.to[lo[j]];
        } else {
            at[j] = t.at[lo[j]];
        }
        m[j] = t.len[lo[j]] / W;
    }
    u64 to[K];
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u64 elements = at[j] + (u64)u[j] * (16u * W), planes = at[j] + 16ull * u[j]; // plane p: + p * m
        if constexpr (TB::PICKS) to[j] = JOIN ? out_at[j] + (u64)u[j] * (16u * W) : out_at[j] + 16ull * u[j];
        else to[j] = JOIN ? elements : planes;
        if constexpr (PRED != 0) prev[j] = 0; // the predictor restarts with the item
        if (!GUARD || base + (u64)j * RCX_TYPED_ROW + tid < total) {
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(src + (JOIN ? planes + (u64)i * m[j] : elements + 16ull * i), &w[j][4 * i]);
            if constexpr (PRED != 0) {
                if (u[j]) prev[j] = rcx_load_elem<W>(src + elements - W);
            }
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || base + (u64)j * RCX_TYPED_ROW + tid < total) {
            u32 o[4 * W];
            if constexpr (W == 1) {
#pragma unroll
                for (u32 i = 0; i < 4; ++i) o[i] = w[j][i];
            } else if constexpr (PRED != 0) {
                u32 d[4 * W];
                rcx_predict_unit<W, PRED == 2>(w[j], prev[j], d);
                rcx_planes_unit<W, JOIN>(d, o);
            } else {
                rcx_planes_unit<W, JOIN>(w[j], o);
            }
#pragma unroll
            for (u32 i = 0; i < W; ++i)
                rcx_store16<true>(dst + to[j] + (JOIN ? 16ull * i : (u64)i * m[j]), U4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]});
        }
    }
}

// Rest lane r of a class of width W: byte r % 17W of the class's entry r / 17W, if it has one.
template <u32 W, bool JOIN, u32 PRED, class TB>
__device__ __forceinline__ void rcx_typed_rest(const u8* __restrict__ src, u8* __restrict__ dst, const TB& t, u32 first, u32 count, u64 r)
{
    constexpr u32 PER = 17u * W;
    const u64 k = r / PER;
    if (k >= count) return;
    const u32 j = (u32)(r - k * PER), len = t.len[first + k], m = len / W;
    u64 at;
    if constexpr (TB::PICKS) { // (the entry lies elsewhere in dst; join: without a predictor only)
        static_assert(!TB::PICKS || !JOIN || PRED == 0, "a device-planned join with a predictor is the scan kernel's");
        at = t.from[first + k];
        const u64 to = t.to[first + k];
        u32 e, p;
        const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
        if constexpr (JOIN) {
            if (kind == 1) dst[to + (u64)e * W + p] = src[at + (u64)p * m + e];
            else if (kind == 2) dst[to + e] = src[at + e];
        } else { // split: the element, or its difference against the one in front of it (0 in front of the entry), to its planes
            if (kind == 1) {
                if constexpr (PRED != 0) {
                    typedef typename RcxElem<W>::T T;
                    const u8* element = src + at + (u64)e * W;
                    const T here = rcx_load_elem<W>(element), front = e ? rcx_load_elem<W>(element - W) : (T)0;
                    const T d = (T)(here - front) & rcx_elem_mask<W>();
                    dst[to + (u64)p * m + e] = (u8)((PRED == 2 ? rcx_zigzag<W>(d) : d) >> (8u * p));
                } else {
                    dst[to + (u64)p * m + e] = src[at + (u64)e * W + p];
                }
            } else if (kind == 2) {
                dst[to + e] = src[at + e];
            }
        }
        return;
    } else {
        at = t.at[first + k];
    }
    u32 e, p;
    const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
    if (kind == 1) {
        if constexpr (PRED != 0) {
            typedef typename RcxElem<W>::T T;
            const u8* element = src + at + (u64)e * W;
            const T here = rcx_load_elem<W>(element), front = e ? rcx_load_elem<W>(element - W) : (T)0;
            const T d = (T)(here - front) & rcx_elem_mask<W>();
            dst[at + (u64)p * m + e] = (u8)((PRED == 2 ? rcx_zigzag<W>(d) : d) >> (8u * p));
        } else {
            const u64 element = at + (u64)e * W + p, plane = at + (u64)p * m + e;
            dst[JOIN ? element : plane] = src[JOIN ? plane : element];
        }
    } else if (kind == 2) {
        dst[at + e] = src[at + e];
    }
}

// ===========================================================================
// Split (every class), and join of the classes without a predictor.  A fixed grid loops over the steps, then over the
// blocks of rest lanes; the class of a step or block is found on scalars and branched on once.
// ===========================================================================
// (rcx_typed_picks_items_k and rcx_typed_split_picks_k below repeat these two loops for the device-planned tables: a change
// here goes to both of them too)
template <bool JOIN>
__global__ __launch_bounds__(RCX_PLANES_THREADS) void rcx_typed_items_k(const u8* __restrict__ src, u8* __restrict__ dst, RcxTypedTables t)
{
    const RcxTypedClasses* const cl = t.classes;
    const u32 tid = threadIdx.x;
    const u64 steps = cl->step_end[RCX_TYPED_CLASSES - 1];
    for (u64 s = blockIdx.x; s < steps; s += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->step_end, s);
        const u64 local = s - (c ? cl->step_end[c - 1] : 0);
        const u64 ubase = cl->ubase[c], total = cl->ubase[c + 1] - ubase;
        const u32 rows = cl->row_first[c];
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            constexpr u32 W = decltype(w_)::value, PRED = decltype(p_)::value, K = RCX_PLANES_U4 / W, STEP = K * RCX_TYPED_ROW;
            const u64 base = local * STEP;
            const u32 row0 = rows + (u32)(local * K);
            if (base + STEP <= total) rcx_typed_step<W, JOIN, PRED, false>(src, dst, t, ubase, base, total, row0, tid);
            else rcx_typed_step<W, JOIN, PRED, true>(src, dst, t, ubase, base, total, row0, tid);
        });
    }
    const u64 blocks = cl->rest_end[RCX_TYPED_CLASSES - 1];
    for (u64 b = blockIdx.x; b < blocks; b += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->rest_end, b);
        const u64 r = (b - (c ? cl->rest_end[c - 1] : 0)) * RCX_TYPED_ROW + tid;
        const u32 first = cl->ent_first[c], count = cl->ent_first[c + 1] - first;
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            rcx_typed_rest<decltype(w_)::value, JOIN, decltype(p_)::value>(src, dst, t, first, count, r);
        });
    }
}

// The same walk with the tables the device planned (rcx_typed_picks.hpp): join only, the classes without a predictor.  A
// kernel of its own with the loops written out again, not a shared body: with the loops in a function that both kernels
// inline, the compiler turned the loop tests of the kernel above round, and that kernel is to stay what it was.
// (rcx_typed_split_picks_k below is the third copy, for the split: a change here goes there and above too.)
// (four waves a SIMD, as rcx_typed_items_k<true> has by itself: the second position table costs registers, and at three
// waves the kernel lost 6 % on large items)
__global__ __launch_bounds__(RCX_PLANES_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void rcx_typed_picks_items_k(const u8* __restrict__ src, u8* __restrict__ dst, RcxTypedPickTables t)
{
    constexpr bool JOIN = true;
    const RcxTypedClasses* const cl = t.classes;
    const u32 tid = threadIdx.x;
    const u64 steps = cl->step_end[RCX_TYPED_CLASSES - 1];
    for (u64 s = blockIdx.x; s < steps; s += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->step_end, s);
        const u64 local = s - (c ? cl->step_end[c - 1] : 0);
        const u64 ubase = cl->ubase[c], total = cl->ubase[c + 1] - ubase;
        const u32 rows = cl->row_first[c];
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            constexpr u32 W = decltype(w_)::value, PRED = decltype(p_)::value, K = RCX_PLANES_U4 / W, STEP = K * RCX_TYPED_ROW;
            const u64 base = local * STEP;
            const u32 row0 = rows + (u32)(local * K);
            if (base + STEP <= total) rcx_typed_step<W, JOIN, PRED, false>(src, dst, t, ubase, base, total, row0, tid);
            else rcx_typed_step<W, JOIN, PRED, true>(src, dst, t, ubase, base, total, row0, tid);
        });
    }
    const u64 blocks = cl->rest_end[RCX_TYPED_CLASSES - 1];
    for (u64 b = blockIdx.x; b < blocks; b += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->rest_end, b);
        const u64 r = (b - (c ? cl->rest_end[c - 1] : 0)) * RCX_TYPED_ROW + tid;
        const u32 first = cl->ent_first[c], count = cl->ent_first[c + 1] - first;
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            rcx_typed_rest<decltype(w_)::value, JOIN, decltype(p_)::value>(src, dst, t, first, count, r);
        });
    }
}

// ... and the split over the tables the device planned (rcx_typed_split_picks.hpp): every class, with or without a predictor,
// an entry read at from[k] and written at to[k]; the scan members of the tables are not looked at.  The two loops a third
// time, for the reason above: a change in rcx_typed_items_k goes here and to rcx_typed_picks_items_k too.
__global__ __launch_bounds__(RCX_PLANES_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void rcx_typed_split_picks_k(const u8* __restrict__ src, u8* __restrict__ dst, RcxTypedPickTables t)
{
    constexpr bool JOIN = false;
    const RcxTypedClasses* const cl = t.classes;
    const u32 tid = threadIdx.x;
    const u64 steps = cl->step_end[RCX_TYPED_CLASSES - 1];
    for (u64 s = blockIdx.x; s < steps; s += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->step_end, s);
        const u64 local = s - (c ? cl->step_end[c - 1] : 0);
        const u64 ubase = cl->ubase[c], total = cl->ubase[c + 1] - ubase;
        const u32 rows = cl->row_first[c];
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            constexpr u32 W = decltype(w_)::value, PRED = decltype(p_)::value, K = RCX_PLANES_U4 / W, STEP = K * RCX_TYPED_ROW;
            const u64 base = local * STEP;
            const u32 row0 = rows + (u32)(local * K);
            if (base + STEP <= total) rcx_typed_step<W, JOIN, PRED, false>(src, dst, t, ubase, base, total, row0, tid);
            else rcx_typed_step<W, JOIN, PRED, true>(src, dst, t, ubase, base, total, row0, tid);
        });
    }
    const u64 blocks = cl->rest_end[RCX_TYPED_CLASSES - 1];
    for (u64 b = blockIdx.x; b < blocks; b += gridDim.x) {
        const u32 c = rcx_typed_class_of(cl->rest_end, b);
        const u64 r = (b - (c ? cl->rest_end[c - 1] : 0)) * RCX_TYPED_ROW + tid;
        const u32 first = cl->ent_first[c], count = cl->ent_first[c + 1] - first;
        rcx_typed_dispatch<JOIN>(c, [&](auto w_, auto p_) {
            rcx_typed_rest<decltype(w_)::value, JOIN, decltype(p_)::value>(src, dst, t, first, count, r);
        });
    }
}


// One item of the scan list, by one wave: rcx_predict_join_k's walk of one superblock of m = len / W elements at `at`.
// APART (the tables the device planned): it is written at `out` of dst, not at `at`.
template <u32 W, bool ZIGZAG, bool APART = false>
__device__ __forceinline__ void rcx_typed_scan_item(const u8* __restrict__ src, u8* __restrict__ dst, u64 at, u32 len, u32 lane, [[maybe_unused]] u64 out = 0)
{
    u64 to;
    if constexpr (APART) to = out;
    else to = at;
    typedef typename RcxElem<W>::T T;
    constexpr u32 ROW = RCX_PREDICT_TILE_UNITS * 16u;
    const u32 m = len / W;
    const u32 units = m >> 4, rows = (units + RCX_PREDICT_TILE_UNITS - 1) / RCX_PREDICT_TILE_UNITS;
    const u32 full = units / RCX_PREDICT_TILE_UNITS; // rows in which every lane has a unit
    u32 cur[4 * W], nxt[4 * W];
#pragma unroll
    for (u32 i = 0; i < 4 * W; ++i) cur[i] = nxt[i] = 0;
    T carry = 0; // the predictor restarts with the item
    if (rows) rcx_predict_load_row<W>(src, at, m, 0, lane, cur);
    u32 row = 0;
    const u8* planes = src + at + 16ull * lane; // of the lane's unit in row 0
    u8* elements = dst + to + (u64)lane * (16u * W);
    for (; row + 2 < full; row += 2) { // two tiles a turn while the two rows behind them are whole
        rcx_predict_load_unit<W>(planes + (u64)(row + 1) * ROW, m, nxt);
        rcx_predict_join_tile<W, ZIGZAG>(cur, elements + (u64)row * (ROW * W), true, carry, lane);
        rcx_predict_load_unit<W>(planes + (u64)(row + 2) * ROW, m, cur);
        rcx_predict_join_tile<W, ZIGZAG>(nxt, elements + (u64)(row + 1) * (ROW * W), true, carry, lane);
    }
    for (; row < rows; ++row) { // the last rows, with the tests: the next row is loaded first
        if (row + 1 < rows) rcx_predict_load_row<W>(src, at, m, row + 1, lane, nxt);
        const u32 u = row * RCX_PREDICT_TILE_UNITS + lane;
        rcx_predict_join_tile<W, ZIGZAG>(cur, dst + to + (u64)u * (16u * W), u < units, carry, lane);
#pragma unroll
        for (u32 i = 0; i < 4 * W; ++i) cur[i] = nxt[i];
    }
    const u32 e0 = m & ~15u, left = m - e0; // the last m % 16 elements: the end of the same chain, one element a lane
    if (left) {
        T z = 0;
        if (lane < left) {
#pragma unroll
            for (u32 p = 0; p < W; ++p) z |= (T)src[at + (u64)p * m + e0 + lane] << (8u * p);
        }
        const T upto = rcx_wave_scan<T>(ZIGZAG ? rcx_unzigzag<W>(z) : z, lane);
        if (lane < left) rcx_store_elem<W>(dst + to + (u64)(e0 + lane) * W, (T)(upto + carry) & rcx_elem_mask<W>());
    }
    if (lane < len - m * W) dst[to + (u64)m * W + lane] = src[at + (u64)m * W + lane]; // the tail
}

// ===========================================================================
// Join with a predictor: a workgroup is one wave, a wave owns whole items of the scan list (longest first) and walks
// each tile by tile.  Width and predictor are the item's, the same in all 64 lanes: read, made scalar, branched on.
// ===========================================================================
// (rcx_typed_picks_scan_k below repeats the loop and the switch for the device-planned scan list)
__global__ __launch_bounds__(RCX_PREDICT_TILE_UNITS) void rcx_typed_items_scan_k(const u8* __restrict__ src, u8* __restrict__ dst, RcxTypedTables t)
{
    const u32 lane = threadIdx.x;
    for (u64 i = blockIdx.x; i < t.nscan; i += gridDim.x) {
        const u64 at = t.scan_at[i];
        const u32 len = t.scan_len[i];
        const u32 kind = (u32)__builtin_amdgcn_readfirstlane((int)t.scan_kind[i]);
        switch (kind) {
        case 2u | 16u: rcx_typed_scan_item<2, false>(src, dst, at, len, lane); break;
        case 2u | 32u: rcx_typed_scan_item<2, true>(src, dst, at, len, lane); break;
        case 4u | 16u: rcx_typed_scan_item<4, false>(src, dst, at, len, lane); break;
        case 4u | 32u: rcx_typed_scan_item<4, true>(src, dst, at, len, lane); break;
        case 8u | 16u: rcx_typed_scan_item<8, false>(src, dst, at, len, lane); break;
        default: rcx_typed_scan_item<8, true>(src, dst, at, len, lane); break;
        }
    }
}

// ... over the scan list the device planned: as many waves as the launch has, the list's length read from memory, an item
// read at scan_from and written at scan_to
__global__ __launch_bounds__(RCX_PREDICT_TILE_UNITS) void rcx_typed_picks_scan_k(const u8* __restrict__ src, u8* __restrict__ dst, RcxTypedPickTables t)
{
    const u32 lane = threadIdx.x;
    const u64 nscan = t.nscan[0];
    for (u64 i = blockIdx.x; i < nscan; i += gridDim.x) {
        const u64 at = t.scan_from[i], to = t.scan_to[i];
        const u32 len = t.scan_len[i];
        const u32 kind = (u32)__builtin_amdgcn_readfirstlane((int)t.scan_kind[i]);
        switch (kind) {
        case 2u | 16u: rcx_typed_scan_item<2, false, true>(src, dst, at, len, lane, to); break;
        case 2u | 32u: rcx_typed_scan_item<2, true, true>(src, dst, at, len, lane, to); break;
        case 4u | 16u: rcx_typed_scan_item<4, false, true>(src, dst, at, len, lane, to); break;
        case 4u | 32u: rcx_typed_scan_item<4, true, true>(src, dst, at, len, lane, to); break;
        case 8u | 16u: rcx_typed_scan_item<8, false, true>(src, dst, at, len, lane, to); break;
        default: rcx_typed_scan_item<8, true, true>(src, dst, at, len, lane, to); break;
        }
    }
}

#endif // !RCX_HOST_SIM
