// rcx_stored_api.hpp -- the calls of include/rcx_stored.h on top of the kernels of rcx_stored.hpp.
//
// mix     three steps on the device with no host read between them: sizes and flags per block from the coder's offset table
//         (rcx_stored_sizes_k, into the context's size table, which the block encode call in front has reserved), their
//         prefix sum (rcx_scan_sizes_k as it is: it latches RCX_E_CAPACITY), the copy (rcx_stored_copy_k<RcxMixEntries>).
// decode  the picks are planned on the host as the item decode call plans them, in two parts of one table: the kept picks,
//         longest first, which the coder's decode launches take as they are -- every entry has its own place in d_dst, so
//         they need not follow one another -- and the stored picks, longest first, which one launch of the copy kernel
//         takes.  Either part may be empty.  Without a stored pick the call IS rcx_decode_items_device.
#pragma once

#include "../../include/rcx_stored.h"
#include "rcx_stats_api.hpp"

namespace
{

// workgroups of the copy kernel for `nentries` entries, the first `nlong` long: eight to a compute unit (32 waves, what a
// CU holds), and they loop over the units
u32 stored_copy_grid(const rcx_ctx* c, u64 nentries, u64 nlong)
{
    const u64 units = nlong + (nentries - nlong + RCX_COPY_WAVES - 1) / RCX_COPY_WAVES, most = 8ull * (u64)c->cus;
    return (u32)(units < most ? units : most);
}

// The plan of a decode call: plan_items' checks and order (rcx_items.hpp), the kept picks in front of the stored ones.
// -> *nkept, *nlong (how many of the stored entries, which begin at nkept, are long), *kept_longest.
int plan_stored_picks(const u64* table, u64 count, const u64* pick, u64 nstreams, const u8* stored, ItemPlan& p, u64* nkept, u64* nlong, u32* kept_longest)
{
    if (count > 0x7FFFFFFFull) return RCX_E_ARG;
    std::vector<u64> keys;
    keys.reserve(count);
    const bool sorted = items_sorted();
    u64 kept = 0;
    for (u64 k = 0; k < count; ++k) {
        if (table[k + 1] < table[k] || table[k + 1] - table[k] > RCX_MAX_BLOCK) return RCX_E_ARG;
        const u64 st = pick ? pick[k] : k;
        if (st >= nstreams) return RCX_E_ARG;
        const u32 len = (u32)(table[k + 1] - table[k]);
        if (len == 0) continue;
        const bool raw = stored[st] != 0;
        kept += !raw;
        // ascending keys = the kept picks first, then descending length (or nothing), then the caller's order
        keys.push_back(((u64)raw << 63) | ((u64)(sorted ? 0x00FFFFFFu - len : 0u) << 32) | k);
    }
    std::sort(keys.begin(), keys.end());
    const u64 nwork = keys.size();
    p.nwork = nwork;
    p.at.resize(nwork);
    p.len.resize(nwork);
    p.id.resize(nwork);
    p.stream.resize(nwork);
    p.inv.clear();
    p.classes.clear();
    p.slots_bytes = 0;
    p.longest = 0;
    *kept_longest = 0;
    u32 raw_longest = 0;
    *nlong = 0;
    for (u64 w = 0; w < nwork; ++w) {
        const u64 k = keys[w] & 0xFFFFFFFFull;
        const u32 len = (u32)(table[k + 1] - table[k]);
        p.at[w] = table[k];
        p.len[w] = len;
        p.id[w] = (u32)k;
        p.stream[w] = (u32)(pick ? pick[k] : k);
        if (len > p.longest) p.longest = len;
        if (w < kept) {
            if (len > *kept_longest) *kept_longest = len;
        } else {
            if (len > raw_longest) raw_longest = len;
            if (sorted && len > RCX_COPY_SHORT) *nlong += 1;
        }
    }
    // in the caller's order (diagnostic) every stored entry is taken as long once one is, as rcx_stats_items_device does
    if (!sorted && raw_longest > RCX_COPY_SHORT) *nlong = nwork - kept;
    *nkept = kept;
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_stored_mix_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t block, const void* d_comp, uint64_t comp_size,
                          const uint64_t* d_comp_offsets, uint32_t gain, void* d_dst, uint64_t dst_cap, uint64_t* d_offsets, uint8_t* d_stored,
                          void* stream)
{
    if (!c || !block_ok(block) || gain > 65535u || !d_offsets) return RCX_E_ARG;
    if (n && (!d_src || !d_comp || !d_comp_offsets || !d_dst || !d_stored)) return RCX_E_ARG;
    if (n && (stats_overlap(d_dst, dst_cap, d_src, n) || stats_overlap(d_dst, dst_cap, d_comp, comp_size))) return RCX_E_ARG;
    const u64 nblocks = rcx_block_count(n, block);
    if (nblocks > 0x7FFFFFFFull) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    if (nblocks == 0) return hipMemsetAsync(d_offsets, 0, sizeof(u64), s) == hipSuccess ? RCX_OK : RCX_E_HIP;
    const int r = c->sizes.reserve(nblocks + 1); // (there already behind rcx_encode_blocks_device on the same n and block)
    if (r != RCX_OK) return r;
    {
        const u64 want = (nblocks + 255) / 256, most = 8ull * (u64)c->cus;
        hipLaunchKernelGGL(rcx_stored_sizes_k, dim3((u32)(want < most ? want : most)), dim3(256), 0, s, n, block, nblocks, d_comp_offsets, comp_size,
                           gain, c->sizes.get(), d_stored, c->status.get());
    }
    hipLaunchKernelGGL(rcx_scan_sizes_k, dim3(1), dim3(1024), 0, s, static_cast<const u32*>(c->sizes), nblocks, d_offsets, dst_cap, c->status.get());
    const u64 nlong = block > RCX_COPY_SHORT ? nblocks : 0;
    const RcxMixEntries e{static_cast<const u8*>(d_src), block, static_cast<const u8*>(d_comp), d_comp_offsets, d_stored, d_offsets,
                          static_cast<u8*>(d_dst), dst_cap};
    hipLaunchKernelGGL(rcx_stored_copy_k<RcxMixEntries>, dim3(stored_copy_grid(c, nblocks, nlong)), dim3(RCX_COPY_THREADS), 0, s, nblocks, nlong, e);
    return LAUNCHED();
}

int rcx_stored_decode_device(rcx_ctx* c, int coder, const void* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets, uint64_t nstreams,
                             const uint8_t* stored, const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, void* d_dst, void* stream)
{
    bool any = false;
    if (stored && nstreams <= 0x7FFFFFFFull)
        for (u64 i = 0; i < nstreams && !any; ++i) any = stored[i] != 0;
    if (!any) return rcx_decode_items_device(c, coder, d_comp, comp_size, d_comp_offsets, nstreams, pick, npick, dst_offsets, d_dst, stream);
    if (!c || !coder_ok(coder) || (npick && !dst_offsets)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    ItemPlan& p = c->plan;
    u64 nkept = 0, nlong = 0;
    u32 kept_longest = 0;
    int r = plan_stored_picks(dst_offsets, npick, pick, nstreams, stored, p, &nkept, &nlong, &kept_longest);
    if (r != RCX_OK) return r;
    if (p.nwork == 0) return RCX_OK;
    if (!d_comp || !d_comp_offsets || !d_dst) return RCX_E_ARG;
    if (nkept) {
        if (!is_rans(coder) && (r = ensure_divtab(c, kept_longest)) != RCX_OK) return r;
        if ((r = ensure_redo(c, nkept)) != RCX_OK) return r;
    }
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    if (nkept && (r = decode_launches(c, coder, d_comp, comp_size, d_comp_offsets, nkept, kept_longest, 0, d_dst, s, c->redo, false, g)) != RCX_OK) return r;
    const u64 nraw = p.nwork - nkept;
    if (nraw == 0) return RCX_OK;
    const RcxPickEntries e{static_cast<const u8*>(d_comp), comp_size, d_comp_offsets, static_cast<u8*>(d_dst), c->status.get(), items_from(g, nkept)};
    hipLaunchKernelGGL(rcx_stored_copy_k<RcxPickEntries>, dim3(stored_copy_grid(c, nraw, nlong)), dim3(RCX_COPY_THREADS), 0, s, nraw, nlong, e);
    return LAUNCHED();
}

int rcx_stored_mix(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t block, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets,
                   uint32_t gain, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* offsets, uint8_t* stored)
{
    if (!c || !block_ok(block) || gain > 65535u || !dst_size) return RCX_E_ARG;
    *dst_size = 0;
    if (n && (!src || !comp || !comp_offsets || !dst)) return RCX_E_ARG;
    const u64 nblocks = rcx_block_count(n, block);
    if (nblocks > 0x7FFFFFFFull) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return RCX_OK;
    }
    // staging: the source and the streams in h_in; both tables in h_off; the mixed streams (never more than n) and the flags in h_out
    int r = reserve_staging(c, n + comp_size, n + nblocks, 2 * (nblocks + 1));
    if (r != RCX_OK) return r;
    u8* const d_comp = c->h_in + n;
    u64* const d_out_offsets = c->h_off + (nblocks + 1);
    u8* const d_flags = c->h_out + n;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    if (comp_size) HIP_TRY(hipMemcpy(d_comp, comp, comp_size, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, comp_offsets, (nblocks + 1) * sizeof(u64), hipMemcpyHostToDevice));
    if ((r = rcx_stored_mix_device(c, c->h_in, n, block, d_comp, comp_size, c->h_off, gain, c->h_out, n, d_out_offsets, d_flags, nullptr)) != RCX_OK) return r;
    if ((r = rcx_ctx_sync_status(c, nullptr, nullptr)) != RCX_OK) return r;
    u64 total = 0;
    HIP_TRY(hipMemcpy(&total, d_out_offsets + nblocks, sizeof(u64), hipMemcpyDeviceToHost));
    *dst_size = total;
    if (offsets) HIP_TRY(hipMemcpy(offsets, d_out_offsets, (nblocks + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    if (stored) HIP_TRY(hipMemcpy(stored, d_flags, nblocks, hipMemcpyDeviceToHost));
    if (total > dst_cap) return RCX_E_CAPACITY;
    if (total) HIP_TRY(hipMemcpy(dst, c->h_out, total, hipMemcpyDeviceToHost));
    return RCX_OK;
}

int rcx_stored_decode(rcx_ctx* c, int coder, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets, uint64_t nstreams,
                      const uint8_t* stored, const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, uint8_t* dst, uint64_t dst_cap)
{
    if (!c || !coder_ok(coder) || (npick && !dst_offsets) || (nstreams && !comp_offsets)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (npick == 0) return RCX_OK;
    for (u64 k = 0; k < npick; ++k)
        if (dst_offsets[k + 1] < dst_offsets[k] || dst_offsets[k + 1] - dst_offsets[k] > RCX_MAX_BLOCK || (pick ? pick[k] : k) >= nstreams) return RCX_E_ARG;
    if (dst_offsets[npick] > dst_cap) return RCX_E_CAPACITY;
    const u64 base = dst_offsets[0], n = dst_offsets[npick] - base;
    if (n == 0) return RCX_OK;
    if (!comp || !dst) return RCX_E_ARG;
    int r = reserve_staging(c, comp_size, n, nstreams + 1);
    if (r != RCX_OK) return r;
    std::vector<u64> rel(npick + 1); // the device copy begins at the first pick
    for (u64 k = 0; k <= npick; ++k) rel[k] = dst_offsets[k] - base;
    if (comp_size) HIP_TRY(hipMemcpy(c->h_in, comp, comp_size, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, comp_offsets, (nstreams + 1) * sizeof(u64), hipMemcpyHostToDevice));
    if ((r = rcx_stored_decode_device(c, coder, c->h_in, comp_size, c->h_off, nstreams, stored, pick, npick, rel.data(), c->h_out, nullptr)) != RCX_OK) return r;
    if ((r = rcx_ctx_sync_status(c, nullptr, nullptr)) != RCX_OK) return r;
    HIP_TRY(hipMemcpy(dst + base, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // extern "C"
