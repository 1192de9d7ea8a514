// rcx_typed_split_picks_api.hpp -- the calls of include/rcx_typed_split_picks.h on top of the planner of
// rcx_typed_split_picks.hpp.
//
// rcx_typed_split_picks_device enqueues, and nothing else: the planner's four launches (none of them clears anything: no word
// has to be zero before the first), then rcx_typed_split_picks_k for every class (rcx_typed_items.hpp).  What depends on the
// tables' contents is decided on the device; what the host decides depends on max_pick, max_bytes and the compute units alone.
//
// The scratch is the class planner's for one set, 12 keys and no scan list (rcx_typed_picks_api.hpp, class_plan_in).
#pragma once

#include "../../include/rcx_typed_split_picks.h"
#include "rcx_typed_picks_api.hpp" // tpick_sizes_ok, tpick_apart, class_plan_in, class_plan_launch, picks_staged
#include "rcx_typed_split_picks.hpp"

extern "C" {

uint64_t rcx_typed_split_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes)
{
    if (!tpick_sizes_ok(max_pick, max_bytes) || max_pick == 0) return 0;
    return class_plan_in<RcxTypedSplitPolicy>(nullptr, max_pick, max_bytes, nullptr);
}

int rcx_typed_split_picks_reserve(rcx_ctx* c, uint64_t max_pick, uint64_t max_bytes)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? c->itab.reserve(class_plan_in<RcxTypedSplitPolicy>(nullptr, max_pick, max_bytes, nullptr)) : RCX_OK;
}

int rcx_typed_split_picks_device(rcx_ctx* c, const void* d_src, uint64_t src_cap, const uint64_t* d_src_at, const uint64_t* d_dst_at,
                                 const uint64_t* d_len, const uint8_t* d_widths, const uint8_t* d_preds, const uint64_t* d_count, uint64_t max_pick,
                                 uint64_t max_bytes, void* d_dst, uint64_t dst_cap, uint64_t* d_kept, void* stream)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    if (max_pick == 0) return RCX_OK; // (no table has an entry, a count above 0 is not seen: nothing is enqueued)
    if (!d_src || !d_src_at || !d_dst_at || !d_len || !d_widths || !d_count || !d_dst) return RCX_E_ARG;
    if (!tpick_apart(d_src, src_cap, d_dst, dst_cap)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    const int r = c->itab.reserve(class_plan_in<RcxTypedSplitPolicy>(nullptr, max_pick, max_bytes, nullptr)); // (after rcx_typed_split_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    RcxClassPlan p;
    (void)class_plan_in<RcxTypedSplitPolicy>(c->itab, max_pick, max_bytes, &p);
    const RcxTypedPickIn t{d_src_at, d_dst_at, d_len, d_widths, d_preds, d_count, max_pick, max_bytes, src_cap, dst_cap};
    class_plan_launch<RcxTypedSplitPolicy>(c, s, t, p, max_bytes, d_kept);
    const RcxClassSet& set = p.set[0]; // (nscan[0] is 0: no scan list; the walking launch under RCX_T_ENCODE)
    const RcxTypedPickTables w{set.classes, set.ufirst, set.from, set.to, set.len, set.rowtab, nullptr, nullptr, nullptr, nullptr, p.nscan};
    // the walking kernel's grid, as the host-planned call has it, from what the promise allows: a workgroup step is 64 KiB of
    // any width and each of the 12 classes may have one that is not whole; an entry has at most 17 * 8 rest lanes
    const u64 steps = max_bytes / ((u64)RCX_PLANES_U4 * RCX_TYPED_ROW * 16u) + RCX_TYPED_CLASSES;
    const u64 rests = (max_pick * 17u * 8u + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW + RCX_TYPED_CLASSES;
    const u64 want = steps > rests ? steps : rests, most = 4ull * (u64)c->cus;
    Timed timed(c, s, RCX_T_ENCODE);
    hipLaunchKernelGGL(rcx_typed_split_picks_k, dim3((u32)(want < most ? want : most)), dim3(RCX_PLANES_THREADS), 0, s, static_cast<const u8*>(d_src),
                       static_cast<u8*>(d_dst), w);
    return LAUNCHED();
}

int rcx_typed_split_picks(rcx_ctx* c, const uint8_t* src, uint64_t src_cap, const uint64_t* src_at, const uint64_t* dst_at, const uint64_t* len,
                          const uint8_t* widths, const uint8_t* preds, uint64_t npick, uint8_t* dst, uint64_t dst_cap, uint64_t* kept)
{
    if (!c || npick > 0x7FFFFFFFull || !src || !dst || (npick && (!src_at || !dst_at || !len || !widths))) return RCX_E_ARG;
    if (!tpick_apart(src, src_cap, dst, dst_cap)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (npick == 0) return RCX_OK;
    return picks_staged(
        c, src, src_cap, nullptr, 0, false, src_at, dst_at, len, nullptr, widths, preds, nullptr, npick, dst, dst_cap, kept,
        [&](u64 k) { return rcx_tpick_validate(src_at[k], dst_at[k], len[k], widths[k], preds ? preds[k] : 0u, src_cap, dst_cap) == RCX_TPICK_OK; },
        [&](const PicksStaged& d, u64 max_bytes) {
            return rcx_typed_split_picks_device(c, c->h_in, src_cap, d.from, d.to, d.len, d.widths, d.preds, d.count, npick, max_bytes, c->h_out, dst_cap,
                                                kept ? d.kept : nullptr, nullptr);
        });
}

} // extern "C"
