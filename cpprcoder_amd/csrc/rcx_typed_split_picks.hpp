// rcx_typed_split_picks.hpp -- the planner of rcx_typed_split_picks_device (include/rcx_typed_split_picks.h): what
// rcx_typed_plan(..., scan = false) does on the host (rcx_typed_items.hpp, whose comment block says what the tables must hold)
// for entries that lie in device memory, each with a source and a destination position of its own.  The mirror of
// rcx_typed_picks.hpp, and simpler: the forward predictor is local to an element and the one in front of it, so an entry with a
// predictor is an entry of its class like any other -- no scan list, no bins, no longest-first order, and nothing that has to be
// zero before the first launch.  The kernels are the class planner's (rcx_class_plan.hpp) with 12 class keys, a valid entry's
// key its class of rcx_typed_class (1 and 2 have no entries: width 1 takes no predictor): four launches -- classify, top, apply
// over all max_pick entries with kept[], rows -- and no clear launch.  Then rcx_typed_split_picks_k (rcx_typed_items.hpp) walks
// the tables.
//
// The rules per entry are plain functions, also compiled into tests/sim/typed_split_picks_san.cpp.
#pragma once

#include "rcx_typed_picks.hpp" // rcx_tpick_validate, the class planner

#define RCX_SPICK_KEYS RCX_TYPED_CLASSES // a valid entry's key is its class

#if !defined(RCX_HOST_SIM)

// The split's policy for the class planner: what the call is given is an RcxTypedPickIn, as the join's, and the join's rule
// per entry; kept goes beside it.
struct RcxTypedSplitPolicy {
    typedef RcxTypedPickIn In;
    static constexpr u32 KEYS = RCX_SPICK_KEYS, SETS = 1u, POPULATED[2] = {RCX_TYPED_CLASSES, 0u};
    static constexpr bool SCAN = false, KEPT = true;
    static RCX_DEV u32 classify(const In& t, u64 k, u64 len, u32 w, u32& key)
    {
        const u32 pr = t.preds ? t.preds[k] : 0u;
        const u32 bad = rcx_tpick_validate(t.src_at[k], t.dst_at[k], len, w, pr, t.src_cap, t.dst_cap);
        if (!bad) key = rcx_typed_class(w, pr);
        return bad;
    }
    static RCX_HD u32 set_of(u32) { return 0u; }
    static RCX_HD u32 class_of(u32 key) { return key; }
    static RCX_HD u32 rows(u32, u32 w) { return RCX_PLANES_U4 / w; }
};

#endif // !RCX_HOST_SIM
