// rcx_stored_items_api.hpp -- the calls of include/rcx_stored_items.h on top of the kernels of rcx_stored_items.hpp.
//
// mix     the three steps of rcx_stored_mix_device in item geometry, with no host read between them: sizes and flags per
//         item (rcx_stored_item_sizes_k, into the context's size table in work order), their prefix sum in the caller's order
//         (rcx_scan_sizes_k<RcxItems> as it is: it latches RCX_E_CAPACITY), the copy (rcx_stored_copy_k<RcxMixItemEntries>).
//         The plan is the item encode call's own (plan_items, rcx_items.hpp): the same checks, the same work order, longest
//         first, so the entries above RCX_COPY_SHORT bytes lead it -- also in the diagnostic order, which keeps the length
//         classes together, and RCX_COPY_SHORT is a class border.  All that is added here is their count.
// decode  needs no call: rcx_stored_decode_device (rcx_stored_api.hpp) is in item geometry already.
#pragma once

#include "../../include/rcx_stored_items.h"
#include "rcx_stored_api.hpp"
#include "rcx_stored_items.hpp"

namespace
{

// how many entries of an encode plan a workgroup copies: they are the first ones of the work order
u64 mix_items_long(const ItemPlan& p)
{
    u64 nlong = 0;
    while (nlong < p.nwork && p.len[nlong] > RCX_COPY_SHORT) ++nlong;
    return nlong;
}

} // namespace

extern "C" {

int rcx_stored_mix_items_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, const void* d_comp, uint64_t comp_size,
                                const uint64_t* d_comp_offsets, uint32_t gain, void* d_dst, uint64_t dst_cap, uint64_t* d_offsets, uint8_t* d_stored,
                                void* stream)
{
    if (!c || gain > 65535u || !d_offsets || (nitems && (!src_offsets || !d_stored))) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    ItemPlan& p = c->plan;
    int r = plan_items(RCX_CODER_ADAPTIVE, src_offsets, nitems, nullptr, 0, true, p); // (the coder sizes the slots, which nothing here uses)
    if (r != RCX_OK) return r;
    if (p.nwork == 0) { // no item, or only empty ones: the zero table, no flag set
        HIP_TRY(hipMemsetAsync(d_offsets, 0, (nitems + 1) * sizeof(u64), s));
        if (nitems) HIP_TRY(hipMemsetAsync(d_stored, 0, nitems, s));
        return RCX_OK;
    }
    if (!d_src || !d_comp || !d_comp_offsets || !d_dst) return RCX_E_ARG;
    const u8* const span = static_cast<const u8*>(d_src) + src_offsets[0];
    if (stats_overlap(d_dst, dst_cap, span, src_offsets[nitems] - src_offsets[0]) || stats_overlap(d_dst, dst_cap, d_comp, comp_size)) return RCX_E_ARG;
    if ((r = c->sizes.reserve(p.nwork + 1)) != RCX_OK) return r; // (there already behind rcx_encode_items_device on the same items)
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    {
        const u64 want = (nitems + 255) / 256, most = 8ull * (u64)c->cus;
        hipLaunchKernelGGL(rcx_stored_item_sizes_k, dim3((u32)(want < most ? want : most)), dim3(256), 0, s, nitems, d_comp_offsets, comp_size, gain,
                           c->sizes.get(), d_stored, c->status.get(), g);
    }
    hipLaunchKernelGGL(rcx_scan_sizes_k<RcxItems>, dim3(1), dim3(1024), 0, s, static_cast<const u32*>(c->sizes), nitems, d_offsets, dst_cap,
                       c->status.get(), g);
    const u64 nlong = mix_items_long(p);
    const RcxMixItemEntries e{static_cast<const u8*>(d_src), static_cast<const u8*>(d_comp), d_comp_offsets, d_stored, d_offsets,
                              static_cast<u8*>(d_dst), dst_cap, g};
    hipLaunchKernelGGL(rcx_stored_copy_k<RcxMixItemEntries>, dim3(stored_copy_grid(c, p.nwork, nlong)), dim3(RCX_COPY_THREADS), 0, s, p.nwork, nlong, e);
    return LAUNCHED();
}

int rcx_stored_mix_items(rcx_ctx* c, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems, const uint8_t* comp, uint64_t comp_size,
                         const uint64_t* comp_offsets, uint32_t gain, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* offsets,
                         uint8_t* stored)
{
    if (!c || gain > 65535u || !dst_size || (nitems && !src_offsets) || nitems > 0x7FFFFFFFull) return RCX_E_ARG;
    *dst_size = 0;
    for (u64 i = 0; i < nitems; ++i)
        if (src_offsets[i + 1] < src_offsets[i] || src_offsets[i + 1] - src_offsets[i] > RCX_MAX_BLOCK) return RCX_E_ARG;
    const u64 base = nitems ? src_offsets[0] : 0, n = nitems ? src_offsets[nitems] - base : 0;
    if (n && (!src || !comp || !comp_offsets || !dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) {
        if (offsets) memset(offsets, 0, (nitems + 1) * sizeof(u64));
        if (stored && nitems) memset(stored, 0, nitems);
        return RCX_OK;
    }
    // staging: the items' span and the streams in h_in; both tables in h_off; the mixed streams (never more than n) and the flags in h_out
    int r = reserve_staging(c, n + comp_size, n + nitems, 2 * (nitems + 1));
    if (r != RCX_OK) return r;
    u8* const d_comp = c->h_in + n;
    u64* const d_out_offsets = c->h_off + (nitems + 1);
    u8* const d_flags = c->h_out + n;
    std::vector<u64> rel(nitems + 1); // the device copy begins at the first item
    for (u64 i = 0; i <= nitems; ++i) rel[i] = src_offsets[i] - base;
    HIP_TRY(hipMemcpy(c->h_in, src + base, n, hipMemcpyHostToDevice));
    if (comp_size) HIP_TRY(hipMemcpy(d_comp, comp, comp_size, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, comp_offsets, (nitems + 1) * sizeof(u64), hipMemcpyHostToDevice));
    if ((r = rcx_stored_mix_items_device(c, c->h_in, rel.data(), nitems, d_comp, comp_size, c->h_off, gain, c->h_out, n, d_out_offsets, d_flags, nullptr)) != RCX_OK)
        return r;
    if ((r = rcx_ctx_sync_status(c, nullptr, nullptr)) != RCX_OK) return r;
    u64 total = 0;
    HIP_TRY(hipMemcpy(&total, d_out_offsets + nitems, sizeof(u64), hipMemcpyDeviceToHost));
    *dst_size = total;
    if (offsets) HIP_TRY(hipMemcpy(offsets, d_out_offsets, (nitems + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    if (stored) HIP_TRY(hipMemcpy(stored, d_flags, nitems, hipMemcpyDeviceToHost));
    if (total > dst_cap) return RCX_E_CAPACITY;
    if (total) HIP_TRY(hipMemcpy(dst, c->h_out, total, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // extern "C"
