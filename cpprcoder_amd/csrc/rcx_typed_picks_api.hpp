// rcx_typed_picks_api.hpp -- the calls of include/rcx_typed_picks.h on top of the planner of rcx_typed_picks.hpp.
//
// rcx_typed_join_picks_device enqueues, and nothing else: the planner's five launches (the first clears its counters), then
// rcx_typed_picks_items_k for the entries without a predictor and rcx_typed_picks_scan_k for those with one
// (rcx_typed_items.hpp).  What depends on the tables' contents is decided on the device; what the host decides depends on
// max_pick, max_bytes and the compute units alone.
//
// The scratch, in the context's table scratch (class_plan_in, for every call of the class planner; T tiles, R rows of a set,
// rcx_tpick_tiles / rcx_class_rows_most; "set" once per set, "scan" with a scan list only), the 8-byte tables first:
//     set: head | set: ufirst u64[max_pick + 1] | set: from, to (, bat) u64[max_pick] | scan: scan_from, scan_to u64[max_pick]
//     | tile_sum u64[(KEYS + 1) T] | tile_units u64[KEYS T] | tile_ents u32[KEYS T] | set: len u32[max_pick]
//     | scan: scan_len u32[max_pick] | keys u32[max_pick] | set: rowtab u32[R] | scan: cursor, bins u32[RCX_TPICK_BINS]
//     | nscan u32[2] | scan: scan_kind u8[max_pick]
#pragma once

#include "../../include/rcx_typed_picks.h"
#include "rcx_typed_items_api.hpp"
#include "rcx_typed_picks.hpp"

namespace
{

bool tpick_sizes_ok(u64 max_pick, u64 max_bytes) { return max_pick <= 0x7FFFFFFFull && max_bytes <= RCX_TPICK_MAX_BYTES; }

// the tables of policy P's plan in `base` (nullptr: only their size) -> their bytes
template <class P>
u64 class_plan_in(u8* base, u64 max_pick, u64 max_bytes, RcxClassPlan* p)
{
    const u64 tiles = rcx_tpick_tiles(max_pick);
    u64 o = 0;
    RcxClassPlan q{};
    auto take = [&](auto*& field, u64 count) {
        field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(base + o);
        o += count * sizeof(*field);
    };
    static_assert(sizeof(RcxTypedClasses) % 8 == 0, "the 8-byte tables follow the heads");
    for (u32 s = 0; s < P::SETS; ++s) take(q.set[s].classes, 1);
    for (u32 s = 0; s < P::SETS; ++s) take(q.set[s].ufirst, max_pick + 1);
    for (u32 s = 0; s < P::SETS; ++s) {
        take(q.set[s].from, max_pick);
        take(q.set[s].to, max_pick);
        if (s) take(q.set[s].bat, max_pick);
    }
    if (P::SCAN) take(q.scan_from, max_pick), take(q.scan_to, max_pick);
    take(q.tile_sum, (P::KEYS + 1) * tiles);
    take(q.tile_units, P::KEYS * tiles);
    take(q.tile_ents, P::KEYS * tiles);
    for (u32 s = 0; s < P::SETS; ++s) take(q.set[s].len, max_pick);
    if (P::SCAN) take(q.scan_len, max_pick);
    take(q.keys, max_pick);
    for (u32 s = 0; s < P::SETS; ++s) take(q.set[s].rowtab, rcx_class_rows_most(max_bytes, P::POPULATED[s]));
    if (P::SCAN) take(q.cursor, RCX_TPICK_BINS), take(q.bins, RCX_TPICK_BINS);
    take(q.nscan, 2);
    if (P::SCAN) take(q.scan_kind, max_pick);
    if (p) *p = q;
    return (o + 7) & ~7ull;
}

// policy P's planner launches (with rcx_ctx_set_timing: under RCX_T_SCAN; not under capture)
template <class P>
void class_plan_launch(rcx_ctx* c, hipStream_t s, const typename P::In& t, const RcxClassPlan& p, u64 max_bytes, u64* d_kept)
{
    const u64 tiles = rcx_tpick_tiles(t.max_pick);
    const dim3 grid((u32)(tiles < RCX_TPICK_GRID ? tiles : RCX_TPICK_GRID)), threads(RCX_TPICK_THREADS);
    Timed timed(c, s, RCX_T_SCAN);
    if (P::SCAN) hipLaunchKernelGGL(rcx_class_clear_k, dim3(grid_for(RCX_TPICK_BINS, RCX_TPICK_THREADS)), threads, 0, s, p);
    hipLaunchKernelGGL(rcx_class_classify_k<P>, grid, threads, 0, s, t, p, c->status.get());
    hipLaunchKernelGGL(rcx_class_top_k<P>, dim3(1), dim3(RCX_TPICK_TOP), 0, s, t, p, c->status.get());
    hipLaunchKernelGGL(rcx_class_apply_k<P>, grid, threads, 0, s, t, p, d_kept);
    for (u32 i = 0; i < P::SETS; ++i) {
        const u64 rows = rcx_class_rows_most(max_bytes, P::POPULATED[i]), groups = (rows + RCX_TPICK_THREADS - 1) / RCX_TPICK_THREADS;
        hipLaunchKernelGGL(rcx_class_rows_k, dim3((u32)(groups < RCX_TPICK_GRID ? groups : RCX_TPICK_GRID)), threads, 0, s, p.set[i], rows);
    }
}

// What the host-buffer calls of the three planned calls stage: src, (the base,) the widths, the predictors (and the ops) in
// h_in; the three tables, (the base offsets,) the count (and kept) in h_off; dst in h_out.
struct PicksStaged {
    const u8 *base, *widths, *preds, *ops; // (preds, ops: nullptr where the caller gave none)
    u64 *from, *to, *len, *bat, *count, *kept;
};

// The host-buffer call of a planned call, behind its argument checks: the promise -- what the entries with valid(k) have
// between them --, the staging, enqueue(staged, max_bytes) = the device call, the latched status, dst (and kept) back.
// based: the call has a base, ops and base offsets (base_at is uploaded if given); kept: or nullptr.
template <class Valid, class Enqueue>
int picks_staged(rcx_ctx* c, const u8* src, u64 src_cap, const u8* base, u64 base_cap, bool based, const u64* src_at, const u64* dst_at, const u64* len,
                 const u64* base_at, const u8* widths, const u8* preds, const u8* ops, u64 npick, u8* dst, u64 dst_cap, u64* kept, Valid valid, Enqueue enqueue)
{
    u64 max_bytes = 0; // the promise
    for (u64 k = 0; k < npick; ++k)
        if (len[k] && valid(k)) max_bytes += len[k];
    if (max_bytes > RCX_TPICK_MAX_BYTES) return RCX_E_ARG;
    const u64 pad = (npick + 15) & ~15ull;
    const u64 base_in = (src_cap + 15) & ~15ull, widths_at = base_in + ((base_cap + 15) & ~15ull), preds_at = widths_at + pad, ops_at = preds_at + pad;
    int r = reserve_staging(c, (based ? ops_at : preds_at) + npick, dst_cap, (3 + (based ? 1 : 0) + (kept ? 1 : 0)) * npick + 1);
    if (r != RCX_OK) return r;
    PicksStaged d{c->h_in + base_in, c->h_in + widths_at, preds ? c->h_in + preds_at : nullptr, ops ? c->h_in + ops_at : nullptr};
    d.from = c->h_off, d.to = d.from + npick, d.len = d.to + npick, d.bat = d.len + npick;
    d.count = based ? d.bat + npick : d.bat, d.kept = d.count + 1;
    if (src_cap) HIP_TRY(hipMemcpy(c->h_in, src, src_cap, hipMemcpyHostToDevice));
    if (base_cap) HIP_TRY(hipMemcpy(c->h_in + base_in, base, base_cap, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_in + widths_at, widths, npick, hipMemcpyHostToDevice));
    if (preds) HIP_TRY(hipMemcpy(c->h_in + preds_at, preds, npick, hipMemcpyHostToDevice));
    if (ops) HIP_TRY(hipMemcpy(c->h_in + ops_at, ops, npick, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.from, src_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.to, dst_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.len, len, npick * sizeof(u64), hipMemcpyHostToDevice));
    if (base_at) HIP_TRY(hipMemcpy(d.bat, base_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.count, &npick, sizeof(u64), hipMemcpyHostToDevice));
    if (dst_cap) HIP_TRY(hipMemcpy(c->h_out, dst, dst_cap, hipMemcpyHostToDevice)); // (what no entry writes stays as it is)
    r = enqueue(d, max_bytes);
    if (r != RCX_OK) return r;
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (dst_cap) HIP_TRY(hipMemcpy(dst, c->h_out, dst_cap, hipMemcpyDeviceToHost)); // (the good entries also behind a latched failure)
    if (kept) HIP_TRY(hipMemcpy(kept, d.kept, npick * sizeof(u64), hipMemcpyDeviceToHost));
    return r;
}

bool tpick_apart(const void* a, u64 na, const void* b, u64 nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x <= y ? y - x >= na : x - y >= nb; // the two ranges are apart (or touch)
}

} // namespace

extern "C" {

uint64_t rcx_typed_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes)
{
    if (!tpick_sizes_ok(max_pick, max_bytes) || max_pick == 0) return 0;
    return class_plan_in<RcxTypedJoinPolicy>(nullptr, max_pick, max_bytes, nullptr);
}

int rcx_typed_picks_reserve(rcx_ctx* c, uint64_t max_pick, uint64_t max_bytes)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? c->itab.reserve(class_plan_in<RcxTypedJoinPolicy>(nullptr, max_pick, max_bytes, nullptr)) : RCX_OK;
}

int rcx_typed_join_picks_device(rcx_ctx* c, const void* d_src, uint64_t src_cap, const uint64_t* d_src_at, const uint64_t* d_dst_at,
                                const uint64_t* d_len, const uint8_t* d_widths, const uint8_t* d_preds, const uint64_t* d_count, uint64_t max_pick,
                                uint64_t max_bytes, void* d_dst, uint64_t dst_cap, void* stream)
{
    if (!c || !tpick_sizes_ok(max_pick, max_bytes)) return RCX_E_ARG;
    if (max_pick == 0) return RCX_OK; // (no table has an entry, a count above 0 is not seen: nothing is enqueued)
    if (!d_src || !d_src_at || !d_dst_at || !d_len || !d_widths || !d_count || !d_dst) return RCX_E_ARG;
    if (!tpick_apart(d_src, src_cap, d_dst, dst_cap)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    const int r = c->itab.reserve(class_plan_in<RcxTypedJoinPolicy>(nullptr, max_pick, max_bytes, nullptr)); // (after rcx_typed_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    RcxClassPlan p;
    (void)class_plan_in<RcxTypedJoinPolicy>(c->itab, max_pick, max_bytes, &p);
    const RcxTypedPickIn t{d_src_at, d_dst_at, d_len, d_widths, d_preds, d_count, max_pick, max_bytes, src_cap, dst_cap};
    class_plan_launch<RcxTypedJoinPolicy>(c, s, t, p, max_bytes, nullptr);
    const RcxClassSet& set = p.set[0]; // (the walking launches under RCX_T_DECODE)
    const RcxTypedPickTables w{set.classes, set.ufirst, set.from, set.to, set.len, set.rowtab, p.scan_from, p.scan_to, p.scan_len, p.scan_kind, p.nscan};
    // the walking kernels' grids, as the host-planned call has them, from what the promise allows: a workgroup step is 64 KiB
    // of any width, an entry has at most 17 * 8 rest lanes; a wave to an item of the scan list
    const u64 steps = max_bytes / ((u64)RCX_PLANES_U4 * RCX_TYPED_ROW * 16u) + 4, rests = (max_pick * 17u * 8u + RCX_TYPED_ROW - 1) / RCX_TYPED_ROW + 4;
    const u64 want = steps > rests ? steps : rests, most = 4ull * (u64)c->cus, waves = 32ull * (u64)c->cus;
    const u8* const src = static_cast<const u8*>(d_src);
    u8* const dst = static_cast<u8*>(d_dst);
    Timed timed(c, s, RCX_T_DECODE);
    hipLaunchKernelGGL(rcx_typed_picks_items_k, dim3((u32)(want < most ? want : most)), dim3(RCX_PLANES_THREADS), 0, s, src, dst, w);
    if (d_preds) hipLaunchKernelGGL(rcx_typed_picks_scan_k, dim3((u32)(max_pick < waves ? max_pick : waves)), dim3(RCX_PREDICT_TILE_UNITS), 0, s, src, dst, w);
    return LAUNCHED();
}

int rcx_typed_join_picks(rcx_ctx* c, const uint8_t* src, uint64_t src_cap, const uint64_t* src_at, const uint64_t* dst_at, const uint64_t* len,
                         const uint8_t* widths, const uint8_t* preds, uint64_t npick, uint8_t* dst, uint64_t dst_cap)
{
    if (!c || npick > 0x7FFFFFFFull || !src || !dst || (npick && (!src_at || !dst_at || !len || !widths))) return RCX_E_ARG;
    if (!tpick_apart(src, src_cap, dst, dst_cap)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (npick == 0) return RCX_OK;
    return picks_staged(
        c, src, src_cap, nullptr, 0, false, src_at, dst_at, len, nullptr, widths, preds, nullptr, npick, dst, dst_cap, nullptr,
        [&](u64 k) { return rcx_tpick_validate(src_at[k], dst_at[k], len[k], widths[k], preds ? preds[k] : 0u, src_cap, dst_cap) == RCX_TPICK_OK; },
        [&](const PicksStaged& d, u64 max_bytes) {
            return rcx_typed_join_picks_device(c, c->h_in, src_cap, d.from, d.to, d.len, d.widths, d.preds, d.count, npick, max_bytes, c->h_out, dst_cap, nullptr);
        });
}

} // extern "C"
