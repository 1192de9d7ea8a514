// rcx_typed_split_picks_api.hpp -- the calls of include/rcx_typed_split_picks.h on top of the planner of
// rcx_typed_split_picks.hpp.
//
// rcx_typed_split_picks_device enqueues, and nothing else: the planner's four launches (none of them clears anything: no word
// has to be zero before the first), then rcx_typed_split_picks_k for every class (rcx_typed_items.hpp).  What depends on the
// tables' contents is decided on the device; what the host decides depends on max_pick, max_bytes and the compute units alone.
//
// The scratch, in the context's table scratch (T tiles, R rows, rcx_tpick_tiles / rcx_spick_rows_most):
//     head | ufirst u64[max_pick + 1] | from, to u64[max_pick] | tile_sum u64[13 T] | tile_units u64[12 T] | tile_ents u32[12 T]
//     | len, keys u32[max_pick] | rowtab u32[R] | over u32[2]
#pragma once

#include "../../include/rcx_typed_split_picks.h"
#include "rcx_typed_picks_api.hpp" // tpick_sizes_ok, tpick_apart
#include "rcx_typed_split_picks.hpp"

namespace
{

// the tables in `base` (nullptr: only their size) -> their bytes
u64 spick_plan_in(u8* base, u64 max_pick, u64 max_bytes, RcxTypedSplitPickPlan* p)
{
    const u64 tiles = rcx_tpick_tiles(max_pick), rows = rcx_spick_rows_most(max_bytes);
    u64 o = 0;
    RcxTypedSplitPickPlan q;
    auto take = [&](auto*& field, u64 count) {
        field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(base + o);
        o += count * sizeof(*field);
    };
    take(q.classes, 1);
    take(q.ufirst, max_pick + 1);
    take(q.from, max_pick);
    take(q.to, max_pick);
    take(q.tile_sum, RCX_SPICK_SUMS * tiles);
    take(q.tile_units, RCX_SPICK_KEYS * tiles);
    take(q.tile_ents, RCX_SPICK_KEYS * tiles);
    take(q.len, max_pick);
    take(q.keys, max_pick);
    take(q.rowtab, rows);
    take(q.over, 2);
    if (p) *p = q;
    return (o + 7) & ~7ull;
}

} // namespace

extern "C" {

uint64_t rcx_typed_split_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes)
{
    if (!tpick_sizes_ok(max_pick, max_bytes) || max_pick == 0) return 0;
    return spick_plan_in(nullptr, max_pick, max_bytes, nullptr);
}

int rcx_typed_split_picks_reserve(rcx_ctx* c, uint64_t max_pick, uint64_t max_bytes)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? c->itab.reserve(spick_plan_in(nullptr, max_pick, max_bytes, nullptr)) : RCX_OK;
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
    const int r = c->itab.reserve(spick_plan_in(nullptr, max_pick, max_bytes, nullptr)); // (after rcx_typed_split_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    RcxTypedSplitPickPlan p;
    (void)spick_plan_in(c->itab, max_pick, max_bytes, &p);
    const RcxTypedPickIn t{d_src_at, d_dst_at, d_len, d_widths, d_preds, d_count, max_pick, max_bytes, src_cap, dst_cap};
    const u64 tiles = rcx_tpick_tiles(max_pick), rows = rcx_spick_rows_most(max_bytes);
    const u32 grid = (u32)(tiles < RCX_TPICK_GRID ? tiles : RCX_TPICK_GRID);
    const u64 row_groups = (rows + RCX_TPICK_THREADS - 1) / RCX_TPICK_THREADS;
    RcxTypedPickPlan rp{}; // rcx_tpick_rows_k as it is: it reads the three fields that are set here
    rp.classes = p.classes, rp.ufirst = p.ufirst, rp.rowtab = p.rowtab;
    { // (with rcx_ctx_set_timing: the planner under RCX_T_SCAN, the walking launch under RCX_T_ENCODE; not under capture)
        Timed timed(c, s, RCX_T_SCAN);
        hipLaunchKernelGGL(rcx_spick_classify_k, dim3(grid), dim3(RCX_TPICK_THREADS), 0, s, t, p, c->status.get());
        hipLaunchKernelGGL(rcx_spick_top_k, dim3(1), dim3(RCX_TPICK_TOP), 0, s, t, p, c->status.get());
        hipLaunchKernelGGL(rcx_spick_apply_k, dim3(grid), dim3(RCX_TPICK_THREADS), 0, s, t, p, d_kept);
        hipLaunchKernelGGL(rcx_tpick_rows_k, dim3((u32)(row_groups < RCX_TPICK_GRID ? row_groups : RCX_TPICK_GRID)), dim3(RCX_TPICK_THREADS), 0, s, rp, rows);
    }
    const RcxTypedPickTables w{p.classes, p.ufirst, p.from, p.to, p.len, p.rowtab, nullptr, nullptr, nullptr, nullptr, p.over + 1};
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
    u64 max_bytes = 0; // the promise: what the valid entries have between them
    for (u64 k = 0; k < npick; ++k)
        if (len[k] && rcx_tpick_validate(src_at[k], dst_at[k], len[k], widths[k], preds ? preds[k] : 0u, src_cap, dst_cap) == RCX_TPICK_OK) max_bytes += len[k];
    if (max_bytes > RCX_TPICK_MAX_BYTES) return RCX_E_ARG;
    // staging: src, the widths and the predictors in h_in; the three tables, the count and kept in h_off; dst in h_out
    const u64 widths_at = (src_cap + 15) & ~15ull, preds_at = widths_at + ((npick + 15) & ~15ull);
    int r = reserve_staging(c, preds_at + npick, dst_cap, 4 * npick + 1);
    if (r != RCX_OK) return r;
    u64* const d_from = c->h_off;
    u64* const d_to = d_from + npick;
    u64* const d_len = d_to + npick;
    u64* const d_count = d_len + npick;
    u64* const d_kept = d_count + 1;
    if (src_cap) HIP_TRY(hipMemcpy(c->h_in, src, src_cap, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_in + widths_at, widths, npick, hipMemcpyHostToDevice));
    if (preds) HIP_TRY(hipMemcpy(c->h_in + preds_at, preds, npick, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_from, src_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_to, dst_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, len, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, &npick, sizeof(u64), hipMemcpyHostToDevice));
    if (dst_cap) HIP_TRY(hipMemcpy(c->h_out, dst, dst_cap, hipMemcpyHostToDevice)); // (what no entry writes stays as it is)
    r = rcx_typed_split_picks_device(c, c->h_in, src_cap, d_from, d_to, d_len, c->h_in + widths_at, preds ? c->h_in + preds_at : nullptr, d_count, npick,
                                     max_bytes, c->h_out, dst_cap, kept ? d_kept : nullptr, nullptr);
    if (r != RCX_OK) return r;
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (dst_cap) HIP_TRY(hipMemcpy(dst, c->h_out, dst_cap, hipMemcpyDeviceToHost)); // (the good entries also behind a latched failure)
    if (kept) HIP_TRY(hipMemcpy(kept, d_kept, npick * sizeof(u64), hipMemcpyDeviceToHost));
    return r;
}

} // extern "C"
