// rcx_base_picks_api.hpp -- the calls of include/rcx_base_picks.h on top of the planner of rcx_base_picks.hpp.
//
// rcx_base_join_picks_device enqueues, and nothing else: the planner's six launches (the first clears its counters, the last
// two make the two row tables), then rcx_typed_picks_items_k and, with d_preds, rcx_typed_picks_scan_k on the typed set
// (rcx_typed_items.hpp, as rcx_typed_picks_api.hpp launches them) and, with d_ops, rcx_base_picks_items_k on the base set:
// nine at the most, one after the other on one stream.  What depends on the tables' contents is decided on the device; what
// the host decides depends on max_pick, max_bytes, which of d_preds and d_ops are given, and the compute units alone.
//
// The scratch, in the context's table scratch (T tiles, R = rcx_tpick_rows_most, Rb = rcx_bpick_rows_most):
//     head, base head | ufirst, bufirst u64[max_pick + 1] | from, to, bfrom, bto, bat, scan_from, scan_to u64[max_pick]
//     | tile_sum u64[17 T] | tile_units u64[16 T] | tile_ents u32[16 T] | len, blen, scan_len, keys u32[max_pick] | rowtab u32[R]
//     | browtab u32[Rb] | cursor, bins u32[RCX_TPICK_BINS] | nscan u32[2] | scan_kind u8[max_pick]
#pragma once

#include "../../include/rcx_base_picks.h"
#include "rcx_base_items_api.hpp"
#include "rcx_base_picks.hpp"
#include "rcx_typed_picks_api.hpp" // tpick_sizes_ok, tpick_apart

namespace
{

// the tables in `base` (nullptr: only their size) -> their bytes
u64 bpick_plan_in(u8* base, u64 max_pick, u64 max_bytes, RcxBasePickPlan* p)
{
    const u64 tiles = rcx_tpick_tiles(max_pick);
    u64 o = 0;
    RcxBasePickPlan q;
    auto take = [&](auto*& field, u64 count) {
        field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(base + o);
        o += count * sizeof(*field);
    };
    take(q.classes, 1);
    take(q.bclasses, 1);
    take(q.ufirst, max_pick + 1);
    take(q.bufirst, max_pick + 1);
    take(q.from, max_pick);
    take(q.to, max_pick);
    take(q.bfrom, max_pick);
    take(q.bto, max_pick);
    take(q.bat, max_pick);
    take(q.scan_from, max_pick);
    take(q.scan_to, max_pick);
    take(q.tile_sum, RCX_BPICK_SUMS * tiles);
    take(q.tile_units, RCX_BPICK_KEYS * tiles);
    take(q.tile_ents, RCX_BPICK_KEYS * tiles);
    take(q.len, max_pick);
    take(q.blen, max_pick);
    take(q.scan_len, max_pick);
    take(q.keys, max_pick);
    take(q.rowtab, rcx_tpick_rows_most(max_bytes));
    take(q.browtab, rcx_bpick_rows_most(max_bytes));
    take(q.cursor, RCX_TPICK_BINS);
    take(q.bins, RCX_TPICK_BINS);
    take(q.nscan, 2);
    take(q.scan_kind, max_pick);
    if (p) *p = q;
    return (o + 7) & ~7ull;
}

} // namespace

extern "C" {

uint64_t rcx_base_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes)
{
    if (!tpick_sizes_ok(max_pick, max_bytes) || max_pick == 0) return 0;
    return bpick_plan_in(nullptr, max_pick, max_bytes, nullptr);
}

int rcx_base_picks_reserve(rcx_ctx* c, uint64_t max_pick, uint64_t max_bytes)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? c->itab.reserve(bpick_plan_in(nullptr, max_pick, max_bytes, nullptr)) : RCX_OK;
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
    const int r = c->itab.reserve(bpick_plan_in(nullptr, max_pick, max_bytes, nullptr)); // (after rcx_base_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    RcxBasePickPlan p;
    (void)bpick_plan_in(c->itab, max_pick, max_bytes, &p);
    const bool based = d_ops != nullptr;
    const RcxBasePickIn t{d_src_at, based && base_cap > 0 ? d_base_at : nullptr, d_dst_at, d_len, d_widths, d_preds, d_ops, d_count, max_pick, max_bytes,
                          src_cap, based ? base_cap : 0, dst_cap};
    const u64 tiles = rcx_tpick_tiles(max_pick), rows = rcx_tpick_rows_most(max_bytes), brows = rcx_bpick_rows_most(max_bytes);
    const u32 grid = (u32)(tiles < RCX_TPICK_GRID ? tiles : RCX_TPICK_GRID);
    // rcx_tpick_clear_k and rcx_tpick_rows_k as they are: each reads the few fields of its plan that are set here
    RcxTypedPickPlan tp{}, bp{};
    tp.classes = p.classes, tp.ufirst = p.ufirst, tp.rowtab = p.rowtab, tp.bins = p.bins, tp.nscan = p.nscan;
    bp.classes = p.bclasses, bp.ufirst = p.bufirst, bp.rowtab = p.browtab;
    auto row_grid = [](u64 n) {
        const u64 groups = (n + RCX_TPICK_THREADS - 1) / RCX_TPICK_THREADS;
        return dim3((u32)(groups < RCX_TPICK_GRID ? groups : RCX_TPICK_GRID));
    };
    { // (with rcx_ctx_set_timing: the planner under RCX_T_SCAN, the walking launches under RCX_T_DECODE; not under capture)
        Timed timed(c, s, RCX_T_SCAN);
        hipLaunchKernelGGL(rcx_tpick_clear_k, dim3(grid_for(RCX_TPICK_BINS, RCX_TPICK_THREADS)), dim3(RCX_TPICK_THREADS), 0, s, tp);
        hipLaunchKernelGGL(rcx_bpick_classify_k, dim3(grid), dim3(RCX_TPICK_THREADS), 0, s, t, p, c->status.get());
        hipLaunchKernelGGL(rcx_bpick_top_k, dim3(1), dim3(RCX_TPICK_TOP), 0, s, t, p, c->status.get());
        hipLaunchKernelGGL(rcx_bpick_apply_k, dim3(grid), dim3(RCX_TPICK_THREADS), 0, s, t, p);
        hipLaunchKernelGGL(rcx_tpick_rows_k, row_grid(rows), dim3(RCX_TPICK_THREADS), 0, s, tp, rows);
        hipLaunchKernelGGL(rcx_tpick_rows_k, row_grid(brows), dim3(RCX_TPICK_THREADS), 0, s, bp, brows);
    }
    const RcxTypedPickTables w{p.classes, p.ufirst, p.from, p.to, p.len, p.rowtab, p.scan_from, p.scan_to, p.scan_len, p.scan_kind, p.nscan};
    const RcxBasePickTables bw{p.bclasses, p.bufirst, p.bfrom, p.bto, p.bat, p.blen, p.browtab};
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
    u64 max_bytes = 0; // the promise: what the valid entries have between them
    for (u64 k = 0; k < npick; ++k) {
        const u32 op = ops ? ops[k] : RCX_BASE_NONE_OP;
        if (len[k] && rcx_bpick_validate(src_at[k], dst_at[k], op != RCX_BASE_NONE_OP && based ? base_at[k] : 0, len[k], widths[k], preds ? preds[k] : 0u, op, src_cap,
                                         dst_cap, base_cap) == RCX_TPICK_OK)
            max_bytes += len[k];
    }
    if (max_bytes > RCX_TPICK_MAX_BYTES) return RCX_E_ARG;
    // staging: src, the base, the widths, the predictors and the ops in h_in; the four tables and the count in h_off; dst in h_out
    const u64 pad = (npick + 15) & ~15ull;
    const u64 base_in = (src_cap + 15) & ~15ull, widths_at = base_in + ((base_cap + 15) & ~15ull), preds_at = widths_at + pad, ops_at = preds_at + pad;
    int r = reserve_staging(c, ops_at + npick, dst_cap, 4 * npick + 1);
    if (r != RCX_OK) return r;
    u64* const d_from = c->h_off;
    u64* const d_to = d_from + npick;
    u64* const d_len = d_to + npick;
    u64* const d_bat = d_len + npick;
    u64* const d_count = d_bat + npick;
    if (src_cap) HIP_TRY(hipMemcpy(c->h_in, src, src_cap, hipMemcpyHostToDevice));
    if (base_cap) HIP_TRY(hipMemcpy(c->h_in + base_in, base, base_cap, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_in + widths_at, widths, npick, hipMemcpyHostToDevice));
    if (preds) HIP_TRY(hipMemcpy(c->h_in + preds_at, preds, npick, hipMemcpyHostToDevice));
    if (ops) HIP_TRY(hipMemcpy(c->h_in + ops_at, ops, npick, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_from, src_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_to, dst_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, len, npick * sizeof(u64), hipMemcpyHostToDevice));
    if (based) HIP_TRY(hipMemcpy(d_bat, base_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, &npick, sizeof(u64), hipMemcpyHostToDevice));
    if (dst_cap) HIP_TRY(hipMemcpy(c->h_out, dst, dst_cap, hipMemcpyHostToDevice)); // (what no entry writes stays as it is)
    r = rcx_base_join_picks_device(c, c->h_in, src_cap, c->h_in + base_in, base_cap, d_from, d_bat, d_to, d_len, c->h_in + widths_at,
                                   preds ? c->h_in + preds_at : nullptr, ops ? c->h_in + ops_at : nullptr, d_count, npick, max_bytes, c->h_out, dst_cap, nullptr);
    if (r != RCX_OK) return r;
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (dst_cap) HIP_TRY(hipMemcpy(dst, c->h_out, dst_cap, hipMemcpyDeviceToHost)); // (the good entries also behind a latched failure)
    return r;
}

} // extern "C"
