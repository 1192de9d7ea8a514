// rcx_base_items_api.hpp -- the calls of include/rcx_base_items.h: residuals against a base per item.  Everything that
// depends on the items is planned on the host (rcx_base_items.hpp, rcx_base_items_plan) before anything is enqueued, and
// both sets of tables go up inside the call in one copy, into the context's item tables (itab): then rcx_typed_items_k
// and, for join, rcx_typed_items_scan_k on the items without an op, exactly as rcx_typed_items_api.hpp launches them, and
// rcx_base_items_k on those with one.  A kernel whose set is empty is not launched.  Nothing is latched.  The calls cannot
// be captured: the tables are the call's own.
#pragma once

#include "../../include/rcx_base_items.h"
#include "rcx_base_items.hpp"
#include "rcx_ctx.hpp"
#include "rcx_typed_items_api.hpp" // typed_items_check, typed_items_apart

namespace
{

// RCX_E_ARG for what include/rcx_base_items.h refuses in the tables; *n = the bytes the call moves, [*lo, *hi) = the hull of
// the base spans in use (items with an op and with bytes), 0 and 0 where there is none
int base_items_check(const u64* offs, const u64* boffs, const u8* widths, const u8* preds, const u8* ops, u64 nitems, u64* n, u64* lo, u64* hi)
{
    *lo = *hi = 0;
    const int r = typed_items_check(offs, widths, preds, nitems, n);
    if (r != RCX_OK || !ops) return r;
    bool any = false;
    for (u64 i = 0; i < nitems; ++i) {
        const u32 op = ops[i];
        if (op == RCX_BASE_NONE) continue;
        if (op > RCX_BASE_SUBZZ || (preds && preds[i] != RCX_PRED_NONE)) return RCX_E_ARG;
        const u64 len = offs[i + 1] - offs[i];
        if (len == 0) continue;
        if (!boffs || boffs[i] + len < boffs[i]) return RCX_E_ARG;
        if (!any || boffs[i] < *lo) *lo = boffs[i];
        if (!any || boffs[i] + len > *hi) *hi = boffs[i] + len;
        any = true;
    }
    return RCX_OK;
}

// [a + a0, a + a0 + an) and [b + b0, b + b0 + bn) are apart (or touch); an empty range is apart from everything
bool base_items_apart(const void* a, u64 a0, u64 an, const void* b, u64 b0, u64 bn)
{
    if (an == 0 || bn == 0) return true;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a) + a0, y = reinterpret_cast<uintptr_t>(b) + b0;
    return x < y ? y - x >= an : x - y >= bn;
}

template <bool JOIN>
int base_items_launch(rcx_ctx* c, const u8* src, const u8* ref, const u64* offs, const u64* boffs, const u8* widths, const u8* preds, const u8* ops, u64 nitems,
                      u8* dst, hipStream_t s)
{
    RcxBaseItemsPlan p;
    if (!rcx_base_items_plan(offs, boffs, widths, preds, ops, nitems, JOIN, c->itab_host, p)) return RCX_E_ARG;
    const int r = c->itab.reserve(p.bytes);
    if (r != RCX_OK) return r;
    // (a pageable source: the runtime has taken the bytes when the call returns, so the next call may refill itab_host)
    HIP_TRY(hipMemcpyAsync(c->itab, c->itab_host.data(), p.bytes, hipMemcpyHostToDevice, s));
    const RcxTypedTables t = rcx_typed_tables(c->itab, p.typed);
    const RcxBaseItemsTables bt = rcx_base_items_tables(c->itab, p);
    // the grids of rcx_typed_items_api.hpp: four workgroups to a compute unit that loop, fewer where there is less to do
    const u64 most = 4ull * (u64)c->cus;
    const u64 want = p.typed.steps > p.typed.rest_blocks ? p.typed.steps : p.typed.rest_blocks;
    if (want) hipLaunchKernelGGL(rcx_typed_items_k<JOIN>, dim3((u32)(want < most ? want : most)), dim3(RCX_PLANES_THREADS), 0, s, src, dst, t);
    if (JOIN && p.typed.nscan) {
        const u64 waves = 32ull * (u64)c->cus;
        hipLaunchKernelGGL(rcx_typed_items_scan_k, dim3((u32)(p.typed.nscan < waves ? p.typed.nscan : waves)), dim3(RCX_PREDICT_TILE_UNITS), 0, s, src, dst, t);
    }
    const u64 theirs = p.based.steps > p.based.rest_blocks ? p.based.steps : p.based.rest_blocks;
    if (theirs) hipLaunchKernelGGL(rcx_base_items_k<JOIN>, dim3((u32)(theirs < most ? theirs : most)), dim3(RCX_BASE_THREADS), 0, s, src, ref, dst, bt);
    return LAUNCHED();
}

template <bool JOIN>
int base_items_device(rcx_ctx* c, const void* d_src, const void* d_base, const u64* offs, const u64* boffs, const u8* widths, const u8* preds, const u8* ops,
                      u64 nitems, void* d_dst, void* stream)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0, lo = 0, hi = 0;
    const int r = base_items_check(offs, boffs, widths, preds, ops, nitems, &n, &lo, &hi);
    if (r != RCX_OK) return r;
    if (n && (!d_src || !d_dst || !typed_items_apart(d_src, d_dst, offs[0], n))) return RCX_E_ARG;
    if (hi > lo && (!d_base || !base_items_apart(d_dst, offs[0], n, d_base, lo, hi - lo))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return base_items_launch<JOIN>(c, static_cast<const u8*>(d_src), static_cast<const u8*>(d_base), offs, boffs, widths, preds, ops, nitems,
                                   static_cast<u8*>(d_dst), static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int base_items_host(rcx_ctx* c, const uint8_t* src, const uint8_t* ref, u64 ref_bytes, const u64* offs, const u64* boffs, const u8* widths, const u8* preds,
                    const u8* ops, u64 nitems, uint8_t* dst)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0, lo = 0, hi = 0;
    int r = base_items_check(offs, boffs, widths, preds, ops, nitems, &n, &lo, &hi);
    if (r != RCX_OK) return r;
    if (n && (!src || !dst || !typed_items_apart(src, dst, offs[0], n))) return RCX_E_ARG;
    if (hi > lo && (!ref || hi > ref_bytes || !base_items_apart(dst, offs[0], n, ref, lo, hi - lo))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    // the input buffer holds the items and, from the next 16-byte border on, the hull of the base spans in use
    const u64 ref_at = (n + 15) & ~(u64)15;
    if ((r = reserve_staging(c, ref_at + (hi - lo), n, 0)) != RCX_OK) return r;
    const u64 first = offs[0];
    std::vector<u64> rel(nitems + 1), brel(hi > lo ? nitems : 0); // the device copies begin at the first item and at the hull
    for (u64 i = 0; i <= nitems; ++i) rel[i] = offs[i] - first;
    for (u64 i = 0; i < brel.size(); ++i) brel[i] = ops[i] != RCX_BASE_NONE && offs[i + 1] > offs[i] ? boffs[i] - lo : 0;
    HIP_TRY(hipMemcpy(c->h_in, src + first, n, hipMemcpyHostToDevice));
    if (hi > lo) HIP_TRY(hipMemcpy(c->h_in + ref_at, ref + lo, hi - lo, hipMemcpyHostToDevice));
    if ((r = base_items_launch<JOIN>(c, c->h_in, c->h_in + ref_at, rel.data(), brel.data(), widths, preds, ops, nitems, c->h_out, nullptr)) != RCX_OK) return r;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst + first, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_base_items_check(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                         uint64_t nitems)
{
    u64 n = 0, lo = 0, hi = 0;
    return base_items_check(src_offsets, base_offsets, widths, preds, ops, nitems, &n, &lo, &hi);
}

int rcx_base_items_hull(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                        uint64_t nitems, uint64_t* lo, uint64_t* hi)
{
    if (!lo || !hi) return RCX_E_ARG;
    u64 n = 0;
    return base_items_check(src_offsets, base_offsets, widths, preds, ops, nitems, &n, lo, hi);
}

int rcx_base_items_split_device(rcx_ctx* c, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                                const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, void* d_dst, void* stream)
{
    return base_items_device<false>(c, d_src, d_base, src_offsets, base_offsets, widths, preds, ops, nitems, d_dst, stream);
}

int rcx_base_items_join_device(rcx_ctx* c, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                               const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, void* d_dst, void* stream)
{
    return base_items_device<true>(c, d_src, d_base, src_offsets, base_offsets, widths, preds, ops, nitems, d_dst, stream);
}

int rcx_base_items_split(rcx_ctx* c, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets, const uint64_t* base_offsets,
                         const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, uint8_t* dst)
{
    return base_items_host<false>(c, src, base, base_bytes, src_offsets, base_offsets, widths, preds, ops, nitems, dst);
}

int rcx_base_items_join(rcx_ctx* c, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets, const uint64_t* base_offsets,
                        const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, uint8_t* dst)
{
    return base_items_host<true>(c, src, base, base_bytes, src_offsets, base_offsets, widths, preds, ops, nitems, dst);
}

} // extern "C"
