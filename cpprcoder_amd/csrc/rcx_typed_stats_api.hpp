// rcx_typed_stats_api.hpp -- the calls of include/rcx_typed_stats.h: the cost of every asked candidate of every item.  The
// tables are checked and planned on the host (rcx_typed_stats.hpp, rcx_typed_stats_plan) before anything is enqueued, go up
// inside the call in one copy, into the context's item tables (itab), and rcx_typed_stats_k<W> is launched once per width
// that has entries: at most four launches, whatever the item count.  Nothing is latched.  The calls cannot be captured: the
// tables are the call's own.
#pragma once

#include "../../include/rcx_typed_stats.h"
#include "rcx_base_items_api.hpp" // base_items_apart
#include "rcx_ctx.hpp"
#include "rcx_typed_items_api.hpp" // typed_items_check
#include "rcx_typed_stats.hpp"

namespace
{

// RCX_E_ARG for what include/rcx_typed_stats.h refuses in the tables; *n = the bytes of the items, [*lo, *hi) = the hull of the
// base spans in use (items with an op bit and with bytes), 0 and 0 where there is none
int typed_stats_check(const u64* offs, const u64* boffs, const u8* widths, const u8* masks, u64 nitems, u64* n, u64* lo, u64* hi)
{
    *lo = *hi = 0;
    const int r = typed_items_check(offs, widths, nullptr, nitems, n);
    if (r != RCX_OK || nitems == 0) return r;
    if (!masks) return RCX_E_ARG;
    bool any = false;
    for (u64 i = 0; i < nitems; ++i) {
        const u32 mask = masks[i];
        if (mask >> RCX_CANDS || (widths[i] == 1 && (mask & RCX_TSTATS_PRED_BITS))) return RCX_E_ARG;
        const u64 len = offs[i + 1] - offs[i];
        if (!(mask & RCX_TSTATS_OP_BITS) || len == 0) continue;
        if (!boffs || boffs[i] + len < boffs[i]) return RCX_E_ARG;
        if (!any || boffs[i] < *lo) *lo = boffs[i];
        if (!any || boffs[i] + len > *hi) *hi = boffs[i] + len;
        any = true;
    }
    return RCX_OK;
}

// workgroups of width W a compute unit holds: by its 32 waves, by the kernel's registers and by the table sets in 160 KiB of LDS
template <u32 W>
constexpr u64 typed_stats_per_cu()
{
    return W == 8 ? 3 : W == 4 ? 5 : 8;
}

template <u32 W>
void typed_stats_launch_width(rcx_ctx* c, const u8* src, const u8* ref, const RcxTypedStatsTables& t, u32 first, u32 count, u64* cost, hipStream_t s)
{
    if (!count) return;
    const u64 most = typed_stats_per_cu<W>() * (u64)c->cus;
    hipLaunchKernelGGL(rcx_typed_stats_k<W>, dim3((u32)(count < most ? count : most)), dim3(RCX_TSTATS_THREADS), 0, s, src, ref, t, first, count, cost);
}

int typed_stats_launch(rcx_ctx* c, const u8* src, const u8* ref, const u64* offs, const u64* boffs, const u8* widths, const u8* masks, u64 nitems, u64* cost,
                       hipStream_t s)
{
    RcxTypedStatsPlan p;
    rcx_typed_stats_plan(offs, boffs, widths, masks, nitems, c->itab_host, p);
    const int r = c->itab.reserve(p.bytes);
    if (r != RCX_OK) return r;
    // (a pageable source: the runtime has taken the bytes when the call returns, so the next call may refill itab_host)
    HIP_TRY(hipMemcpyAsync(c->itab, c->itab_host.data(), p.bytes, hipMemcpyHostToDevice, s));
    const RcxTypedStatsTables t = rcx_typed_stats_tables(c->itab, p);
    typed_stats_launch_width<1>(c, src, ref, t, p.first[0], p.first[1] - p.first[0], cost, s);
    typed_stats_launch_width<2>(c, src, ref, t, p.first[1], p.first[2] - p.first[1], cost, s);
    typed_stats_launch_width<4>(c, src, ref, t, p.first[2], p.first[3] - p.first[2], cost, s);
    typed_stats_launch_width<8>(c, src, ref, t, p.first[3], p.first[4] - p.first[3], cost, s);
    return LAUNCHED();
}

} // namespace

extern "C" {

int rcx_typed_stats_check(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* masks, uint64_t nitems)
{
    u64 n = 0, lo = 0, hi = 0;
    return typed_stats_check(src_offsets, base_offsets, widths, masks, nitems, &n, &lo, &hi);
}

int rcx_typed_stats_items_device(rcx_ctx* c, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                                 const uint8_t* widths, const uint8_t* masks, uint64_t nitems, uint64_t* d_cost, void* stream)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0, lo = 0, hi = 0;
    const int r = typed_stats_check(src_offsets, base_offsets, widths, masks, nitems, &n, &lo, &hi);
    if (r != RCX_OK) return r;
    const u64 table = nitems * RCX_CANDS * sizeof(u64);
    if (nitems && (!d_cost || (reinterpret_cast<uintptr_t>(d_cost) & 7u))) return RCX_E_ARG;
    if (n && (!d_src || !base_items_apart(d_cost, 0, table, d_src, src_offsets[0], n))) return RCX_E_ARG;
    if (hi > lo && (!d_base || !base_items_apart(d_cost, 0, table, d_base, lo, hi - lo))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    return typed_stats_launch(c, static_cast<const u8*>(d_src), static_cast<const u8*>(d_base), src_offsets, base_offsets, widths, masks, nitems, d_cost,
                              static_cast<hipStream_t>(stream));
}

int rcx_typed_stats_items(rcx_ctx* c, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets,
                          const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* masks, uint64_t nitems, uint64_t* cost)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0, lo = 0, hi = 0;
    int r = typed_stats_check(src_offsets, base_offsets, widths, masks, nitems, &n, &lo, &hi);
    if (r != RCX_OK) return r;
    const u64 table = nitems * RCX_CANDS * sizeof(u64);
    if (nitems && (!cost || (reinterpret_cast<uintptr_t>(cost) & 7u))) return RCX_E_ARG;
    if (n && (!src || !base_items_apart(cost, 0, table, src, src_offsets[0], n))) return RCX_E_ARG;
    if (hi > lo && (!base || hi > base_bytes || !base_items_apart(cost, 0, table, base, lo, hi - lo))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    // the input buffer holds the items and, from the next 16-byte border on, the hull of the base spans in use
    const u64 ref_at = (n + 15) & ~(u64)15;
    if ((r = reserve_staging(c, ref_at + (hi - lo), table, 0)) != RCX_OK) return r;
    const u64 first = src_offsets[0];
    std::vector<u64> rel(nitems + 1), brel(hi > lo ? nitems : 0); // the device copies begin at the first item and at the hull
    for (u64 i = 0; i <= nitems; ++i) rel[i] = src_offsets[i] - first;
    for (u64 i = 0; i < brel.size(); ++i) brel[i] = (masks[i] & RCX_TSTATS_OP_BITS) && src_offsets[i + 1] > src_offsets[i] ? base_offsets[i] - lo : 0;
    if (n) HIP_TRY(hipMemcpy(c->h_in, src + first, n, hipMemcpyHostToDevice));
    if (hi > lo) HIP_TRY(hipMemcpy(c->h_in + ref_at, base + lo, hi - lo, hipMemcpyHostToDevice));
    if ((r = typed_stats_launch(c, c->h_in, c->h_in + ref_at, rel.data(), hi > lo ? brel.data() : nullptr, widths, masks, nitems,
                                reinterpret_cast<u64*>(c->h_out.get()), nullptr)) != RCX_OK)
        return r;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(cost, c->h_out, table, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // extern "C"
