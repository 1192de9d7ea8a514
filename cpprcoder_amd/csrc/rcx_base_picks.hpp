// rcx_base_picks.hpp -- the planner of rcx_base_join_picks_device (include/rcx_base_picks.h): what rcx_base_items_plan(...,
// scan = true) does on the host (rcx_base_items.hpp) for entries that lie in device memory, each with a source, a base and a
// destination position of its own; and the kernel that walks the base set it leaves.  The plan has the host plan's two sets:
//   the typed set   the entries WITHOUT an op: 4 classes by width and the scan list for those with a predictor -- the tables
//                   rcx_typed_picks.hpp's planner makes when the entries with an op are left out, word for word
//   the base set    the entries WITH an op: 12 classes, 3 * log2(width) + op, a workgroup step of RCX_BASE_ROWS(width) rows,
//                   ufirst, from, to, len, rowtab and bat[k] = the entry's offset in the base
//
// ONE pass of the class planner (rcx_class_plan.hpp) for both sets, with 16 class keys: key 0 .. 3 = the typed classes, 4 .. 15
// = 4 + the base class, 16 + bin = the scan list.  A planner per set would read every entry twice and validate it twice; one
// classify kernel with 16 sums a tile reads an entry once, and the 16 scans are registers and cross-lane moves, which the
// planner has to spare: it is bound by its table reads.  Six launches: clear, classify, top, apply, and the rows of each set.
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

// The join's policy for the class planner: keys 0 .. 3 = class 3 * key of set 0, 4 .. 15 = class key - 4 of set 1.
struct RcxBaseJoinPolicy {
    typedef RcxBasePickIn In;
    static constexpr u32 KEYS = RCX_BPICK_KEYS, SETS = 2u, POPULATED[2] = {RCX_BPICK_TYPED, RCX_TYPED_CLASSES};
    static constexpr bool SCAN = true, KEPT = false;
    static RCX_DEV u32 classify(const In& t, u64 k, u64 len, u32 w, u32& key)
    {
        const u32 pr = t.preds ? t.preds[k] : 0u, op = t.ops ? t.ops[k] : RCX_BASE_NONE_OP;
        const u64 base_at = op != RCX_BASE_NONE_OP && t.base_at ? t.base_at[k] : 0ull; // (not read for an entry without an op)
        const u32 bad = rcx_bpick_validate(t.src_at[k], t.dst_at[k], base_at, len, w, pr, op, t.src_cap, t.dst_cap, t.base_cap);
        if (!bad) key = rcx_bpick_key((u32)len, w, pr, op);
        return bad;
    }
    static RCX_HD u32 set_of(u32 key) { return key < RCX_BPICK_TYPED ? 0u : 1u; }
    static RCX_HD u32 class_of(u32 key) { return key < RCX_BPICK_TYPED ? 3u * key : key - RCX_BPICK_TYPED; }
    static RCX_HD u32 rows(u32 set, u32 w) { return rcx_base_items_rows(set, w); }
};

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
