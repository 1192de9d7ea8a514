// rcx_base_items.hpp -- residuals against a base per item (include/rcx_base_items.h): the items of rcx_typed_items.hpp, each
// with a width of its own and EITHER a predictor, OR a base op (xor, sub, subzz) against a span of a second buffer, or
// neither.  The arithmetic of a unit is rcx_base.hpp's (rcx_base_unit, rcx_base_elem), the planes and the byte-addressed
// accesses are rcx_planes.hpp's, the tables, their search and the rest lanes are rcx_typed_items.hpp's; here is what is
// new: a plan that makes two sets of tables, and the kernel that walks the second.
//
// THE PLAN (host, rcx_base_items_plan; plain C++, also compiled into tests/sim/base_items_san.cpp).  One counting pass and
// one filling pass over the items make
//   the typed set   the items WITHOUT an op, in the format of rcx_typed_plan -- RcxTypedClasses, ufirst, at, len, rowtab,
//                   for join the scan list -- at the front of the memory, byte for byte what rcx_typed_plan makes of a batch
//                   that has no item with an op.  rcx_typed_items_k<JOIN> and rcx_typed_items_scan_k run on it as they are.
//   the base set    the items WITH an op, behind it: the same fields, with class = 3 * log2(width) + op (twelve, uniform in
//                   width and op, so the kernel branches on the class once a step, on a scalar, and no lane tests a width),
//                   a workgroup step of RCX_BASE_ROWS(width) rows -- source and base together are the 16 16-byte registers
//                   a lane has in flight, as in rcx_base_step -- and one more table, bat[k] = the entry's offset in the base.
// Both go up in one copy.  Split is at most two launches, join at most three (typed rows, scan, base rows), whatever the
// item count; a kernel whose set is empty is not launched.
//
// rcx_base_items_k<JOIN> reads exactly the entries' bytes of src and the same number of bytes at bat[k] of the base, and
// writes exactly the entries' ranges of dst, at any alignment of all three.  Whole elements only are read from the base: the
// tail bytes are copied from the source.  No LDS, no barrier, no flag, no scratch, no floating point, no inline assembly;
// no wave waits for another; all offsets are 64-bit.
#pragma once

#include <cstring>

#include "rcx_base.hpp"
#include "rcx_typed_items.hpp"

#define RCX_BASE_NONE_OP 0xFFu // RCX_BASE_NONE of include/rcx_base_items.h: the item has no base

struct RcxBaseItemsTables {
    RcxTypedTables t; // the base set's classes, ufirst, at, len, rowtab (no scan list)
    const u64* bat;   // [nent] byte offset of the entry's span in the base
    static constexpr bool PICKS = false; // (no member: the tables a kernel is handed stay as they are)
};

// The base set as the planner of rcx_base_picks.hpp leaves it in device memory: an entry is read at from[k] of the source and
// bat[k] of the base and written at to[k].  rcx_base_items_step and rcx_base_items_rest take either kind (TB).
struct RcxBasePickTables {
    const RcxTypedClasses* classes;
    const u64* ufirst; // [nent + 1]
    const u64* from;   // [nent] byte offset of the entry in src
    const u64* to;     // [nent] ... in dst
    const u64* bat;    // [nent] ... of its span in the base
    const u32* len;
    const u32* rowtab;
    static constexpr bool PICKS = true;
};

struct RcxBaseItemsPlan {
    RcxTypedPlan typed; // the set of the items without an op: rcx_typed_plan's, at 0
    RcxTypedPlan based; // the set of the items with one; its offsets count from the beginning of the memory as well
    u64 o_based = 0;    // where its classes lie
    u64 o_bat = 0;
    u64 bytes = 0;      // of both
};

// rows of a workgroup step: set 0 = rcx_typed_step's, set 1 = rcx_base_items_step's
RCX_HD u32 rcx_base_items_rows(u32 set, u32 w) { return set ? (u32)RCX_BASE_ROWS(w) : RCX_PLANES_U4 / w; }

// Item i = [offs[i], offs[i + 1]) with widths[i], preds[i] (nullptr = none) and ops[i] (nullptr = none) against
// [boffs[i], boffs[i] + len) of the base, all checked before.  scan = true (join): the entries with a predictor go to the
// scan list, as in rcx_typed_plan.  false if a table outgrows its 32-bit index.
inline bool rcx_base_items_plan(const u64* offs, const u64* boffs, const u8* widths, const u8* preds, const u8* ops, u64 nitems, bool scan,
                                std::vector<u64>& mem, RcxBaseItemsPlan& p)
{
    constexpr u32 NC = RCX_TYPED_CLASSES;
    u64 nent[2][NC] = {}, units[2][NC] = {};
    std::vector<u64> keys; // the scan list: ascending keys = descending length, then the caller's order
    for (u64 i = 0; i < nitems; ++i) {
        const u64 len = offs[i + 1] - offs[i];
        if (len == 0) continue;
        const u32 w = widths[i], op = ops ? ops[i] : RCX_BASE_NONE_OP, pr = preds ? preds[i] : 0u;
        const u32 set = op != RCX_BASE_NONE_OP;
        if (!set && scan && pr) {
            keys.push_back(((u64)(0xFFFFFFFFu - (u32)len) << 32) | i);
            continue;
        }
        const u32 c = rcx_typed_class(w, set ? op : pr);
        nent[set][c] += 1;
        units[set][c] += (len / w) >> 4;
    }
    if (nitems > 0x7FFFFFFFull) return false;
    rcx_typed_longest_first(keys);
    RcxTypedClasses cl[2] = {};
    RcxTypedPlan* const plan[2] = {&p.typed, &p.based};
    u64 o = 0;
    for (u32 set = 0; set < 2; ++set) {
        u64 ents = 0, rows = 0, ub = 0, steps = 0, rests = 0;
        for (u32 c = 0; c < NC; ++c) {
            const u32 w = rcx_typed_class_width(c);
            cl[set].ent_first[c] = (u32)ents;
            cl[set].row_first[c] = (u32)rows;
            cl[set].ubase[c] = ub;
            const u64 step = (u64)rcx_base_items_rows(set, w) * RCX_TYPED_ROW;
            steps += (units[set][c] + step - 1) / step;
            rests += (nent[set][c] * (17u * w) + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
            cl[set].step_end[c] = steps;
            cl[set].rest_end[c] = rests;
            ents += nent[set][c];
            ub += units[set][c];
            if (nent[set][c]) rows += (units[set][c] + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW + 1;
        }
        if (rows > 0x7FFFFFFFull) return false;
        cl[set].ent_first[NC] = (u32)ents;
        cl[set].row_first[NC] = (u32)rows;
        cl[set].ubase[NC] = ub;
        RcxTypedPlan& q = *plan[set];
        q = RcxTypedPlan();
        q.nent = ents;
        q.nrows = rows;
        q.nscan = set ? 0 : keys.size();
        q.steps = steps;
        q.rest_blocks = rests;
        // the 8-byte tables first, then the 4-byte ones, then the bytes: set 0 exactly as rcx_typed_plan lays them out
        if (set) p.o_based = o;
        o += (sizeof(RcxTypedClasses) + 7) & ~(u64)7;
        q.o_ufirst = o, o += (ents + 1) * sizeof(u64);
        q.o_at = o, o += ents * sizeof(u64);
        if (set) p.o_bat = o, o += ents * sizeof(u64);
        q.o_scan_at = o, o += q.nscan * sizeof(u64);
        q.o_len = o, o += ents * sizeof(u32);
        q.o_rowtab = o, o += rows * sizeof(u32);
        q.o_scan_len = o, o += q.nscan * sizeof(u32);
        q.o_scan_kind = o, o += q.nscan;
        q.bytes = o;
        o = (o + 7) & ~(u64)7;
    }
    p.bytes = p.based.bytes;
    mem.resize((p.bytes + 7) / 8);
    u8* const h = reinterpret_cast<u8*>(mem.data());
    if (p.o_based > p.typed.bytes) memset(h + p.typed.bytes, 0, p.o_based - p.typed.bytes); // (the gap between the sets)
    *reinterpret_cast<RcxTypedClasses*>(h) = cl[0];
    *reinterpret_cast<RcxTypedClasses*>(h + p.o_based) = cl[1];
    u64 *ufirst[2], *at[2], *const bat = reinterpret_cast<u64*>(h + p.o_bat);
    u32 *len[2], *rowtab[2];
    u64 next[2][NC], unit[2][NC];
    for (u32 set = 0; set < 2; ++set) {
        ufirst[set] = reinterpret_cast<u64*>(h + plan[set]->o_ufirst);
        at[set] = reinterpret_cast<u64*>(h + plan[set]->o_at);
        len[set] = reinterpret_cast<u32*>(h + plan[set]->o_len);
        rowtab[set] = reinterpret_cast<u32*>(h + plan[set]->o_rowtab);
        for (u32 c = 0; c < NC; ++c) next[set][c] = cl[set].ent_first[c], unit[set][c] = cl[set].ubase[c];
    }
    for (u64 i = 0; i < nitems; ++i) {
        const u64 n = offs[i + 1] - offs[i];
        const u32 w = widths[i], op = ops ? ops[i] : RCX_BASE_NONE_OP, pr = preds ? preds[i] : 0u;
        const u32 set = op != RCX_BASE_NONE_OP;
        if (n == 0 || (!set && scan && pr)) continue;
        const u32 c = rcx_typed_class(w, set ? op : pr);
        const u64 k = next[set][c]++;
        ufirst[set][k] = unit[set][c];
        at[set][k] = offs[i];
        if (set) bat[k] = boffs[i];
        len[set][k] = (u32)n;
        unit[set][c] += (n / w) >> 4;
    }
    for (u32 set = 0; set < 2; ++set) {
        ufirst[set][plan[set]->nent] = cl[set].ubase[NC];
        for (u32 c = 0; c < NC; ++c) {
            if (!nent[set][c]) continue;
            const u64 nrow = (units[set][c] + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
            const u32 last = cl[set].ent_first[c + 1] - 1u;
            u32 k = cl[set].ent_first[c];
            for (u64 r = 0; r < nrow; ++r) {
                const u64 g = cl[set].ubase[c] + r * RCX_TYPED_ROW;
                while (k < last && ufirst[set][k + 1] <= g) ++k;
                rowtab[set][cl[set].row_first[c] + r] = k;
            }
            rowtab[set][cl[set].row_first[c] + nrow] = last;
        }
    }
    u64* const scan_at = reinterpret_cast<u64*>(h + p.typed.o_scan_at);
    u32* const scan_len = reinterpret_cast<u32*>(h + p.typed.o_scan_len);
    u8* const scan_kind = h + p.typed.o_scan_kind;
    for (u64 s = 0; s < p.typed.nscan; ++s) {
        const u64 i = keys[s] & 0xFFFFFFFFull;
        scan_at[s] = offs[i];
        scan_len[s] = (u32)(offs[i + 1] - offs[i]);
        scan_kind[s] = (u8)(widths[i] | (preds[i] << 4));
    }
    return true;
}

// the base set as the kernel reads it, `base` = where `mem` of rcx_base_items_plan lies (the typed set: rcx_typed_tables(base, p.typed))
inline RcxBaseItemsTables rcx_base_items_tables(const u8* base, const RcxBaseItemsPlan& p)
{
    RcxBaseItemsTables b;
    b.t = rcx_typed_tables(base, p.based);
    b.t.classes = reinterpret_cast<const RcxTypedClasses*>(base + p.o_based);
    b.bat = reinterpret_cast<const u64*>(base + p.o_bat);
    return b;
}

#if !defined(RCX_HOST_SIM)

// f(width, op) as compile-time constants for class c = 3 * log2(width) + op; c is the same in every lane of the workgroup
template <class F>
__device__ __forceinline__ void rcx_base_items_dispatch(u32 c, F f)
{
    typedef std::integral_constant<u32, 0> C0;
    typedef std::integral_constant<u32, 1> C1;
    typedef std::integral_constant<u32, 2> C2;
    typedef std::integral_constant<u32, 4> C4;
    typedef std::integral_constant<u32, 8> C8;
    switch (c) {
    case 0: f(C1{}, C0{}); break;
    case 1: f(C1{}, C1{}); break;
    case 2: f(C1{}, C2{}); break;
    case 3: f(C2{}, C0{}); break;
    case 4: f(C2{}, C1{}); break;
    case 5: f(C2{}, C2{}); break;
    case 6: f(C4{}, C0{}); break;
    case 7: f(C4{}, C1{}); break;
    case 8: f(C4{}, C2{}); break;
    case 9: f(C8{}, C0{}); break;
    case 10: f(C8{}, C1{}); break;
    default: f(C8{}, C2{}); break;
    }
}

// the classes, ufirst, len and rowtab of either kind of tables
__device__ __forceinline__ const RcxTypedTables& rcx_base_items_set(const RcxBaseItemsTables& bt) { return bt.t; }
__device__ __forceinline__ const RcxBasePickTables& rcx_base_items_set(const RcxBasePickTables& bt) { return bt; }

// One step of a workgroup in a class of width W and op OP: rows row0 .. row0 + K - 1 of rowtab, units base + j * 256 + tid of
// the class's `total`.  The K rows' entries are found side by side as in rcx_typed_step; then all loads of source (or
// planes) and base, then the arithmetic in rcx_base_step's order, then the stores.  A width-1 entry is a flat run of units.
// GUARD = false: every unit exists; GUARD = true: the class's last step.
template <u32 W, bool JOIN, u32 OP, bool GUARD, class TB>
__device__ __forceinline__ void rcx_base_items_step(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst, const TB& bt,
                                                    u64 ubase, u64 base, u64 total, u32 row0, u32 tid)
{
    static_assert(!TB::PICKS || JOIN, "device-planned tables are the join's");
    constexpr u32 K = RCX_BASE_ROWS(W);
    const auto& t = rcx_base_items_set(bt);
    u32 w[K][4 * W], b[K][4 * W];
    u64 g[K];
    u32 lo[K], hi[K];
    // A row the class's last step does not have takes the last one it has, and a lane without a unit the class's last
    // unit: both read tables that are there and use nothing of them.
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
    u64 elements[K], planes[K], theirs[K];
    u32 m[K];
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u32 u = (u32)(g[j] - t.ufirst[lo[j]]);
        if constexpr (TB::PICKS) { // (join: the planes are read at `from`, the elements written at `to`)
            const u64 from = t.from[lo[j]], to = t.to[lo[j]];
            m[j] = t.len[lo[j]] / W;
            elements[j] = to + (u64)u * (16u * W);
            planes[j] = from + 16ull * u;
        } else {
            const u64 at = t.at[lo[j]];
            m[j] = t.len[lo[j]] / W;
            elements[j] = at + (u64)u * (16u * W);
            planes[j] = at + 16ull * u; // plane p: + p * m
        }
        theirs[j] = bt.bat[lo[j]] + (u64)u * (16u * W);
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || base + (u64)j * RCX_TYPED_ROW + tid < total) {
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(src + (JOIN ? planes[j] + (u64)i * m[j] : elements[j] + 16ull * i), &w[j][4 * i]);
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(ref + theirs[j] + 16ull * i, &b[j][4 * i]);
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || base + (u64)j * RCX_TYPED_ROW + tid < total) {
            u32 o[4 * W];
            if constexpr (W == 1) {
                rcx_base_unit<1, OP, JOIN>(w[j], b[j], o);
            } else {
                u32 r[4 * W];
                if (JOIN) {
                    rcx_planes_unit<W, true>(w[j], r);
                    rcx_base_unit<W, OP, true>(r, b[j], o);
                } else {
                    rcx_base_unit<W, OP, false>(w[j], b[j], r);
                    rcx_planes_unit<W, false>(r, o);
                }
            }
#pragma unroll
            for (u32 i = 0; i < W; ++i)
                rcx_store16<true>(dst + (JOIN ? elements[j] + 16ull * i : planes[j] + (u64)i * m[j]), U4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]});
        }
    }
}

// Rest lane r of a class of width W: byte r % 17W of the class's entry r / 17W, if it has one.  A byte of an element: the
// lane makes the whole element and writes its one byte of it; a tail byte keeps the source's value.
template <u32 W, bool JOIN, u32 OP, class TB>
__device__ __forceinline__ void rcx_base_items_rest(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst, const TB& bt,
                                                    u32 first, u32 count, u64 r)
{
    constexpr u32 PER = 17u * W;
    const u64 k = r / PER;
    if (k >= count) return;
    if constexpr (TB::PICKS) { // (join only: the entry is read at `from` and written at `to`)
        static_assert(!TB::PICKS || JOIN, "device-planned tables are the join's");
        const u32 j = (u32)(r - k * PER), len = bt.len[first + k], m = len / W;
        const u64 from = bt.from[first + k], to = bt.to[first + k];
        u32 e, p;
        const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
        if (kind == 1) {
            const u64 theirs = bt.bat[first + k] + (u64)e * W;
            if constexpr (W == 1) {
                dst[to + e] = (u8)rcx_base_elem<1, OP, true>(src[from + e], ref[theirs]);
            } else {
                typedef typename RcxElem<W>::T T;
                T x = 0;
#pragma unroll
                for (u32 q = 0; q < W; ++q) x |= (T)src[from + (u64)q * m + e] << (8u * q);
                const u64 v = rcx_base_elem<W, OP, true>(x, rcx_load_elem<W>(ref + theirs));
                dst[to + (u64)e * W + p] = (u8)(v >> (8u * p));
            }
        } else if (kind == 2) {
            dst[to + e] = src[from + e];
        }
        return;
    } else {
        const u32 j = (u32)(r - k * PER), len = bt.t.len[first + k], m = len / W;
        const u64 at = bt.t.at[first + k];
        u32 e, p;
        const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
        if (kind == 1) {
            const u64 element = at + (u64)e * W, theirs = bt.bat[first + k] + (u64)e * W;
            if constexpr (W == 1) {
                dst[element] = (u8)rcx_base_elem<1, OP, JOIN>(src[element], ref[theirs]);
            } else {
                typedef typename RcxElem<W>::T T;
                T x = 0;
                if (JOIN) {
#pragma unroll
                    for (u32 q = 0; q < W; ++q) x |= (T)src[at + (u64)q * m + e] << (8u * q);
                } else {
                    x = rcx_load_elem<W>(src + element);
                }
                const u64 v = rcx_base_elem<W, OP, JOIN>(x, rcx_load_elem<W>(ref + theirs));
                dst[JOIN ? element + p : at + (u64)p * m + e] = (u8)(v >> (8u * p));
            }
        } else if (kind == 2) {
            dst[at + e] = src[at + e];
        }
    }
}

// ===========================================================================
// Both directions of the items with an op.  The grid of rcx_typed_items_k: a fixed one that loops over the steps, then
// over the blocks of rest lanes; the class of a step or block is found on scalars and branched on once.
// ===========================================================================
template <bool JOIN>
__global__ __launch_bounds__(RCX_BASE_THREADS) void rcx_base_items_k(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst,
                                                                     RcxBaseItemsTables bt)
{
    const RcxTypedClasses* const cl = bt.t.classes;
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
