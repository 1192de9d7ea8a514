// rcx_crc_api.hpp -- the CRC-32 calls of include/rcx.h: one launch of rcx_crc32_k (rcx_crc.hpp) per call, over blocks or
// over items, storing the checksums or comparing them with the caller's.
//
// The block calls need nothing from the context but its latch: no scratch, no table, nothing to reserve.  The item
// calls plan on the host like the coder item calls (rcx_items.hpp) and send {offset, length, item} per entry inside the
// call -- EVERY item has an entry here, the empty ones too (their CRC is 0, and a verify call checks that), longest
// first so that the one long chain of a skewed batch starts first.
#pragma once

#include "rcx_items.hpp"

namespace
{

int plan_crc_items(const u64* table, u64 count, ItemPlan& p)
{
    if (count > 0x7FFFFFFFull) return RCX_E_ARG;
    std::vector<u64> keys(count);
    for (u64 k = 0; k < count; ++k) {
        if (table[k + 1] < table[k] || table[k + 1] - table[k] > RCX_MAX_BLOCK) return RCX_E_ARG;
        keys[k] = ((u64)(0xFFFFFFFFu - (u32)(table[k + 1] - table[k])) << 32) | k; // ascending keys = descending length, then the caller's order
    }
    if (items_sorted()) std::sort(keys.begin(), keys.end());
    p.nwork = count;
    p.at.resize(count);
    p.len.resize(count);
    p.id.resize(count);
    p.stream.clear();
    p.inv.clear();
    p.classes.clear();
    p.slots_bytes = 0;
    p.longest = 0;
    for (u64 w = 0; w < count; ++w) {
        const u64 k = keys[w] & 0xFFFFFFFFull;
        p.at[w] = table[k];
        p.len[w] = (u32)(table[k + 1] - table[k]);
        p.id[w] = (u32)k;
        if (p.len[w] > p.longest) p.longest = p.len[w];
    }
    return RCX_OK;
}

// d_expected == nullptr: store to d_crc; else verify
int crc_blocks(rcx_ctx* c, const void* d_src, u64 n, u32 block, u32* d_crc, const u32* d_expected, hipStream_t s)
{
    if (!c || !block_ok(block) || (n && (!d_src || !(d_crc || d_expected)))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return crc_launch(c, d_src, n, block, rcx_block_count(n, block), d_crc, d_expected, s, RcxBlocks{});
}

int crc_items(rcx_ctx* c, const void* d_src, const u64* src_offsets, u64 nitems, u32* d_crc, const u32* d_expected, hipStream_t s)
{
    if (!c || (nitems && (!src_offsets || !(d_crc || d_expected)))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    ItemPlan& p = c->plan;
    int r = plan_crc_items(src_offsets, nitems, p);
    if (r != RCX_OK) return r;
    if (p.longest && !d_src) return RCX_E_ARG;
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    return crc_launch(c, d_src, 0, p.longest, p.nwork, d_crc, d_expected, s, g);
}

// the host-buffer calls behind the copy in: launch, wait, 4 bytes per entry back
int crc_host_finish(rcx_ctx* c, int launched, u64 count, u32* crc)
{
    if (launched != RCX_OK) return launched;
    const int r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(crc, c->h_out, count * sizeof(u32), hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_crc32_blocks_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t block, uint32_t* d_crc, void* stream)
{
    if (n && !d_crc) return RCX_E_ARG;
    return crc_blocks(c, d_src, n, block, d_crc, nullptr, static_cast<hipStream_t>(stream));
}

int rcx_crc32_verify_blocks_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t block, const uint32_t* d_expected, void* stream)
{
    if (n && !d_expected) return RCX_E_ARG;
    return crc_blocks(c, d_src, n, block, nullptr, d_expected, static_cast<hipStream_t>(stream));
}

int rcx_crc32_items_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* d_crc, void* stream)
{
    if (nitems && !d_crc) return RCX_E_ARG;
    return crc_items(c, d_src, src_offsets, nitems, d_crc, nullptr, static_cast<hipStream_t>(stream));
}

int rcx_crc32_verify_items_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, const uint32_t* d_expected,
                                  void* stream)
{
    if (nitems && !d_expected) return RCX_E_ARG;
    return crc_items(c, d_src, src_offsets, nitems, nullptr, d_expected, static_cast<hipStream_t>(stream));
}

int rcx_crc32_blocks(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t block, uint32_t* crc)
{
    if (!c || !block_ok(block) || (n && (!src || !crc))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const u64 nblocks = rcx_block_count(n, block);
    const int r = reserve_staging(c, n, nblocks * sizeof(u32), 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    return crc_host_finish(c, rcx_crc32_blocks_device(c, c->h_in, n, block, reinterpret_cast<u32*>(c->h_out.get()), nullptr), nblocks, crc);
}

int rcx_crc32_items(rcx_ctx* c, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* crc)
{
    if (!c || (nitems && (!src_offsets || !crc))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    for (u64 i = 0; i < nitems; ++i)
        if (src_offsets[i + 1] < src_offsets[i] || src_offsets[i + 1] - src_offsets[i] > RCX_MAX_BLOCK) return RCX_E_ARG;
    const u64 base = src_offsets[0], n = src_offsets[nitems] - base;
    if (n && !src) return RCX_E_ARG;
    const int r = reserve_staging(c, n, nitems * sizeof(u32), 0);
    if (r != RCX_OK) return r;
    std::vector<u64> rel(nitems + 1); // the device copy begins at the first item
    for (u64 i = 0; i <= nitems; ++i) rel[i] = src_offsets[i] - base;
    if (n) HIP_TRY(hipMemcpy(c->h_in, src + base, n, hipMemcpyHostToDevice));
    return crc_host_finish(c, rcx_crc32_items_device(c, c->h_in, rel.data(), nitems, reinterpret_cast<u32*>(c->h_out.get()), nullptr), nitems, crc);
}

} // extern "C"
