// rcx_typed_picks.hpp -- the planner of rcx_typed_join_picks_device (include/rcx_typed_picks.h): what rcx_typed_plan(...,
// scan = true) does on the host (rcx_typed_items.hpp, whose comment block says what the tables must hold) for entries that
// lie in device memory, each with a source and a destination position of its own.  Here are the planner's constants, the
// rules per entry and the join's policy; the kernels are the class planner's (rcx_class_plan.hpp, which says what each of the
// five launches does), with 4 class keys -- an entry's width, without a predictor -- and the scan list for the entries with one.
//
// Then rcx_typed_picks_items_k and rcx_typed_picks_scan_k (rcx_typed_items.hpp) walk the tables.  The scan list's order is a
// counting sort as rcx_picks.hpp's: exact below 512 bytes, 1 part in 256 above; which place of its bin an entry gets differs
// from call to call and no output depends on it.
//
// The rules per entry are plain functions, also compiled into tests/sim/typed_picks_san.cpp.
#pragma once

#include "../../include/rcx_predict.h" // RCX_PRED_*, RCX_MAX_BLOCK
#include "rcx_picks.hpp" // rcx_len_bin
#include "rcx_typed_items.hpp"

#define RCX_TPICK_THREADS 256u                                        // entries of a tile = threads of a planner workgroup
#define RCX_TPICK_GRID 512u                                           // workgroups of the planner's entry kernels at the most: they loop
#define RCX_TPICK_TOP 1024u                                           // tiles a pass of the one workgroup over the tile sums
#define RCX_TPICK_EXACT 512u                                          // scan list: lengths below this have a bin each
#define RCX_TPICK_BINS RCX_LEN_BINS(27u)                              // 5120: an entry has less than 2^27 bytes
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
static_assert(RCX_TPICK_EXACT == RCX_PICK_EXACT, "one bin rule");
RCX_HD u32 rcx_tpick_bin(u32 len) { return rcx_len_bin(len, 27u); }

// the key of a valid entry: 0 .. 3 = the class 3 * key of rcx_typed_class without a predictor, 4 + bin = the scan list
RCX_HD u32 rcx_tpick_key(u32 len, u32 w, u32 pr) { return pr ? 4u + rcx_tpick_bin(len) : (w == 1 ? 0u : w == 2 ? 1u : w == 4 ? 2u : 3u); }
RCX_HD u64 rcx_tpick_units(u32 len, u32 w) { return (u64)((len / w) >> 4); }

RCX_HD u64 rcx_tpick_tiles(u64 entries) { return (entries + RCX_TPICK_THREADS - 1) / RCX_TPICK_THREADS; }

#include "rcx_class_plan.hpp"

#if !defined(RCX_HOST_SIM)

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

// The join's policy for the class planner: key 0 .. 3 = class 3 * key, the one set, a scan list.
struct RcxTypedJoinPolicy {
    typedef RcxTypedPickIn In;
    static constexpr u32 KEYS = 4u, SETS = 1u, POPULATED[2] = {4u, 0u}; // (POPULATED: the classes of a set that can have entries)
    static constexpr bool SCAN = true, KEPT = false;
    static RCX_DEV u32 classify(const In& t, u64 k, u64 len, u32 w, u32& key)
    {
        const u32 pr = t.preds ? t.preds[k] : 0u;
        const u32 bad = rcx_tpick_validate(t.src_at[k], t.dst_at[k], len, w, pr, t.src_cap, t.dst_cap);
        if (!bad) key = rcx_tpick_key((u32)len, w, pr);
        return bad;
    }
    static RCX_HD u32 set_of(u32) { return 0u; }
    static RCX_HD u32 class_of(u32 key) { return 3u * key; }
    static RCX_HD u32 rows(u32, u32 w) { return RCX_PLANES_U4 / w; }
};

#endif // !RCX_HOST_SIM
