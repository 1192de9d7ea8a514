// rcx_typed_items_api.hpp -- the calls of include/rcx_typed_items.h: the typed stage per item.  Everything that depends
// on the items is planned on the host (rcx_typed_items.hpp, rcx_typed_plan) before anything is enqueued, and the tables go
// up inside the call, into the context's item tables (itab, as with the coder item calls): one copy, then one launch of
// rcx_typed_items_k for split; for join one of it for the items without a predictor and one of rcx_typed_items_scan_k for
// those with one.  Nothing is latched.  The calls cannot be captured: the tables are the call's own.
#pragma once

#include "../../include/rcx_typed_items.h"
#include "rcx_ctx.hpp"
#include "rcx_typed_items.hpp"

namespace
{

// RCX_E_ARG for what include/rcx_typed_items.h refuses in the tables; *n = the bytes the call moves
int typed_items_check(const u64* offs, const u8* widths, const u8* preds, u64 nitems, u64* n)
{
    *n = 0;
    if (nitems == 0) return RCX_OK;
    if (!offs || !widths || nitems > 0x7FFFFFFFull) return RCX_E_ARG;
    for (u64 i = 0; i < nitems; ++i) {
        const u32 w = widths[i], pr = preds ? preds[i] : 0u;
        if (!(w == 1 || w == 2 || w == 4 || w == 8) || pr > RCX_PRED_ZIGZAG || (w == 1 && pr != RCX_PRED_NONE)) return RCX_E_ARG;
        if (offs[i + 1] < offs[i]) return RCX_E_ARG;
        const u64 len = offs[i + 1] - offs[i];
        if (len / w + len % w > RCX_MAX_BLOCK) return RCX_E_ARG;
    }
    *n = offs[nitems] - offs[0];
    return RCX_OK;
}

bool typed_items_apart(const void* src, const void* dst, u64 first, u64 n)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) + first, b = reinterpret_cast<uintptr_t>(dst) + first;
    return a < b ? b - a >= n : a - b >= n; // the two ranges are apart (or touch)
}

template <bool JOIN>
int typed_items_launch(rcx_ctx* c, const u8* src, const u64* offs, const u8* widths, const u8* preds, u64 nitems, u8* dst, hipStream_t s)
{
    RcxTypedPlan p;
    if (!rcx_typed_plan(offs, widths, preds, nitems, JOIN, c->itab_host, p)) return RCX_E_ARG;
    const int r = c->itab.reserve(p.bytes);
    if (r != RCX_OK) return r;
    // (a pageable source: the runtime has taken the bytes when the call returns, so the next call may refill itab_host)
    HIP_TRY(hipMemcpyAsync(c->itab, c->itab_host.data(), p.bytes, hipMemcpyHostToDevice, s));
    const RcxTypedTables t = rcx_typed_tables(c->itab, p);
    // the grid of rcx_planes_k: a fixed one, four workgroups to a compute unit, that loops; fewer where there is less to do
    const u64 want = p.steps > p.rest_blocks ? p.steps : p.rest_blocks, most = 4ull * (u64)c->cus;
    if (want) hipLaunchKernelGGL(rcx_typed_items_k<JOIN>, dim3((u32)(want < most ? want : most)), dim3(RCX_PLANES_THREADS), 0, s, src, dst, t);
    if (JOIN && p.nscan) { // a wave to an item; at most 32 waves a compute unit, as rcx_predict_join_k has
        const u64 waves = 32ull * (u64)c->cus;
        hipLaunchKernelGGL(rcx_typed_items_scan_k, dim3((u32)(p.nscan < waves ? p.nscan : waves)), dim3(RCX_PREDICT_TILE_UNITS), 0, s, src, dst, t);
    }
    return LAUNCHED();
}

template <bool JOIN>
int typed_items_device(rcx_ctx* c, const void* d_src, const u64* offs, const u8* widths, const u8* preds, u64 nitems, void* d_dst, void* stream)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0;
    const int r = typed_items_check(offs, widths, preds, nitems, &n);
    if (r != RCX_OK) return r;
    if (n && (!d_src || !d_dst || !typed_items_apart(d_src, d_dst, offs[0], n))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return typed_items_launch<JOIN>(c, static_cast<const u8*>(d_src), offs, widths, preds, nitems, static_cast<u8*>(d_dst), static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int typed_items_host(rcx_ctx* c, const uint8_t* src, const u64* offs, const u8* widths, const u8* preds, u64 nitems, uint8_t* dst)
{
    if (!c) return RCX_E_ARG;
    u64 n = 0;
    int r = typed_items_check(offs, widths, preds, nitems, &n);
    if (r != RCX_OK) return r;
    if (n && (!src || !dst || !typed_items_apart(src, dst, offs[0], n))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    if ((r = reserve_staging(c, n, n, 0)) != RCX_OK) return r;
    const u64 base = offs[0];
    std::vector<u64> rel(nitems + 1); // the device copy begins at the first item
    for (u64 i = 0; i <= nitems; ++i) rel[i] = offs[i] - base;
    HIP_TRY(hipMemcpy(c->h_in, src + base, n, hipMemcpyHostToDevice));
    if ((r = typed_items_launch<JOIN>(c, c->h_in, rel.data(), widths, preds, nitems, c->h_out, nullptr)) != RCX_OK) return r;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst + base, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

uint64_t rcx_typed_items_sub_count(const uint8_t* widths, uint64_t nitems)
{
    if (nitems && !widths) return 0;
    u64 count = 0;
    for (u64 i = 0; i < nitems; ++i) {
        const u32 w = widths[i];
        if (!(w == 1 || w == 2 || w == 4 || w == 8)) return 0;
        count += w;
    }
    return count;
}

int rcx_typed_items_sub_offsets(const uint64_t* src_offsets, const uint8_t* widths, uint64_t nitems, uint64_t* sub_offsets)
{
    if (!sub_offsets || (nitems && !src_offsets)) return RCX_E_ARG;
    u64 n = 0;
    const int r = typed_items_check(src_offsets, widths, nullptr, nitems, &n);
    if (r != RCX_OK) return r;
    u64 k = 0;
    sub_offsets[0] = src_offsets ? src_offsets[0] : 0; // (nitems = 0 allows a null table)
    for (u64 i = 0; i < nitems; ++i) {
        const u32 w = widths[i];
        const u64 len = src_offsets[i + 1] - src_offsets[i], m = len / w;
        for (u32 p = 0; p + 1 < w; ++p, ++k) sub_offsets[k + 1] = sub_offsets[k] + m;
        sub_offsets[k + 1] = src_offsets[i + 1]; // the last plane and the tail
        ++k;
    }
    return RCX_OK;
}

int rcx_typed_items_split_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                                 void* d_dst, void* stream)
{
    return typed_items_device<false>(c, d_src, src_offsets, widths, preds, nitems, d_dst, stream);
}

int rcx_typed_items_join_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                                void* d_dst, void* stream)
{
    return typed_items_device<true>(c, d_src, src_offsets, widths, preds, nitems, d_dst, stream);
}

int rcx_typed_items_split(rcx_ctx* c, const uint8_t* src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                          uint8_t* dst)
{
    return typed_items_host<false>(c, src, src_offsets, widths, preds, nitems, dst);
}

int rcx_typed_items_join(rcx_ctx* c, const uint8_t* src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                         uint8_t* dst)
{
    return typed_items_host<true>(c, src, src_offsets, widths, preds, nitems, dst);
}

} // extern "C"
