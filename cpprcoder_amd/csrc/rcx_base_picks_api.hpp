// rcx_base_picks_api.hpp -- the calls of include/rcx_base_picks.h on top of the planner of rcx_base_picks.hpp.
//
// rcx_base_join_picks_device enqueues, and nothing else: the planner's six launches (the first clears its counters, the last
// two make the two row tables), then rcx_typed_picks_items_k and, with d_preds, rcx_typed_picks_scan_k on the typed set
// (rcx_typed_items.hpp, as rcx_typed_picks_api.hpp launches them) and, with d_ops, rcx_base_picks_items_k on the base set:
// nine at the most, one after the other on one stream.  What depends on the tables' contents is decided on the device; what
// the host decides depends on max_pick, max_bytes, which of d_preds and d_ops are given, and the compute units alone.
//
// The scratch is the class planner's for two sets, 16 keys and a scan list (rcx_typed_picks_api.hpp, class_plan_in).
#pragma once

#include "../../include/rcx_base_picks.h"
#include "rcx_base_items_api.hpp"
#include "rcx_base_picks.hpp"
#include "rcx_typed_picks_api.hpp" // tpick_sizes_ok, tpick_apart, class_plan_in, class_plan_launch, picks_staged

extern "C" {

uint64_t rcx_base_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes)
{
    if (!tpick_sizes_ok(max_pick, max_bytes) || max_pick == 0) return 0;
    return class_plan_in<RcxBaseJoinPolicy>(nullptr, max_pick, max_bytes, nullptr);
}

int rcx_base_picks_reserve(rcx_ctx* c, uint64_t max_pick, uint64_t max_bytes)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? c->itab.reserve(class_plan_in<RcxBaseJoinPolicy>(nullptr, max_pick, max_bytes, nullptr)) : RCX_OK;
}

int rcx_base_join_picks_device(rcx_ctx* c, const void* d_src, uint64_t src_cap, const void* d_base, uint64_t base_cap, const uint64_t* d_src_at,
                               const uint64_t* d_base_at, const uint64_t* d_dst_at, const uint64_t* d_len, const uint8_t* d_widths, const uint8_t* d_preds,
                               const uint8_t* d_ops, const uint64_t* d_count, uint64_t max_pick, uint64_t max_bytes, void* d_dst, uint64_t dst_cap, void* stream)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    if (max_pick == 0) return RCX_OK; // (no table has an entry, a count above 0 is not seen: nothing is enqueued)
    if (!d_src || !d_src_at || !d_dst_at || !d_len || !d_widths || !d_count || !d_dst) return RCX_E_ARG;
    if (d_ops && base_cap > 0 && (!d_base || !d_base_at)) return RCX_E_ARG; // (base_cap = 0: no entry with an op can pass, nothing of the base is read)
    if (!tpick_apart(d_src, src_cap, d_dst, dst_cap)) return RCX_E_ARG;
    if (d_ops && d_base && !tpick_apart(d_base, base_cap, d_dst, dst_cap)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    const int r = c->itab.reserve(class_plan_in<RcxBaseJoinPolicy>(nullptr, max_pick, max_bytes, nullptr)); // (after rcx_base_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    RcxClassPlan p;
    (void)class_plan_in<RcxBaseJoinPolicy>(c->itab, max_pick, max_bytes, &p);
    const bool based = d_ops != nullptr;
    const RcxBasePickIn t{d_src_at, based && base_cap > 0 ? d_base_at : nullptr, d_dst_at, d_len, d_widths, d_preds, d_ops, d_count, max_pick, max_bytes,
                          src_cap, based ? base_cap : 0, dst_cap};
    class_plan_launch<RcxBaseJoinPolicy>(c, s, t, p, max_bytes, nullptr);
    const RcxClassSet &ts = p.set[0], &bs = p.set[1]; // (the walking launches under RCX_T_DECODE)
    const RcxTypedPickTables w{ts.classes, ts.ufirst, ts.from, ts.to, ts.len, ts.rowtab, p.scan_from, p.scan_to, p.scan_len, p.scan_kind, p.nscan};
    const RcxBasePickTables bw{bs.classes, bs.ufirst, bs.from, bs.to, bs.bat, bs.len, bs.rowtab};
    // the walking kernels' grids from what the promise allows: a workgroup step of the typed set is 64 KiB of any width, one of
    // the base set 32 KiB; an entry has at most 17 * 8 rest lanes; a wave to an item of the scan list
    const u64 lanes = (max_pick * 17u * 8u + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW;
    const u64 steps = max_bytes / ((u64)RCX_PLANES_U4 * RCX_TYPED_ROW * 16u) + 4, rests = lanes + 4; // (one more a class: 4 and 12 classes)
    const u64 bsteps = max_bytes / ((u64)RCX_BASE_ROWS(1) * RCX_TYPED_ROW * 16u) + 12, brests = lanes + 12;
    const u64 want = steps > rests ? steps : rests, bwant = bsteps > brests ? bsteps : brests;
    const u64 most = 4ull * (u64)c->cus, waves = 32ull * (u64)c->cus;
    const u8* const src = static_cast<const u8*>(d_src);
    u8* const dst = static_cast<u8*>(d_dst);
    Timed timed(c, s, RCX_T_DECODE);
    hipLaunchKernelGGL(rcx_typed_picks_items_k, dim3((u32)(want < most ? want : most)), dim3(RCX_PLANES_THREADS), 0, s, src, dst, w);
    if (d_preds) hipLaunchKernelGGL(rcx_typed_picks_scan_k, dim3((u32)(max_pick < waves ? max_pick : waves)), dim3(RCX_PREDICT_TILE_UNITS), 0, s, src, dst, w);
    if (based) hipLaunchKernelGGL(rcx_base_picks_items_k, dim3((u32)(bwant < most ? bwant : most)), dim3(RCX_BASE_THREADS), 0, s, src, static_cast<const u8*>(d_base), dst, bw);
    return LAUNCHED();
}

int rcx_base_join_picks(rcx_ctx* c, const uint8_t* src, uint64_t src_cap, const uint8_t* base, uint64_t base_cap, const uint64_t* src_at,
                        const uint64_t* base_at, const uint64_t* dst_at, const uint64_t* len, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                        uint64_t npick, uint8_t* dst, uint64_t dst_cap)
{
    if (!c || npick > 0x7FFFFFFFull || !src || !dst || (npick && (!src_at || !dst_at || !len || !widths))) return RCX_E_ARG;
    if (ops && base_cap > 0 && (!base || (npick && !base_at))) return RCX_E_ARG;
    if (!tpick_apart(src, src_cap, dst, dst_cap) || (ops && base && !tpick_apart(base, base_cap, dst, dst_cap))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (npick == 0) return RCX_OK;
    const bool based = ops && base_cap > 0;
    if (!based) base_cap = 0;
    return picks_staged(
        c, src, src_cap, base, base_cap, true, src_at, dst_at, len, based ? base_at : nullptr, widths, preds, ops, npick, dst, dst_cap, nullptr,
        [&](u64 k) {
            const u32 op = ops ? ops[k] : RCX_BASE_NONE_OP;
            return rcx_bpick_validate(src_at[k], dst_at[k], op != RCX_BASE_NONE_OP && based ? base_at[k] : 0, len[k], widths[k], preds ? preds[k] : 0u, op, src_cap,
                                      dst_cap, base_cap) == RCX_TPICK_OK;
        },
        [&](const PicksStaged& d, u64 max_bytes) {
            return rcx_base_join_picks_device(c, c->h_in, src_cap, d.base, base_cap, d.from, d.bat, d.to, d.len, d.widths, d.preds, d.ops, d.count, npick, max_bytes,
                                              c->h_out, dst_cap, nullptr);
        });
}

} // extern "C"
