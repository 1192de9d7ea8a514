// rcx_stats_api.hpp -- the calls of include/rcx_stats.h: one launch of rcx_stats_k (rcx_stats.hpp) per call, over blocks
// or over items, writing the byte counts, the order-0 costs or both.
//
// The geometry and the host table are those of the CRC-32 calls (rcx_crc_api.hpp): the block calls need nothing from the
// context but its device and compute-unit count; the item calls plan on the host with plan_crc_items -- every item has
// an entry, the empty ones too, longest first -- and send the tables inside the call.  Nothing is latched.
#pragma once

#include "../../include/rcx_stats.h"
#include "rcx_crc_api.hpp"

namespace
{

// [a, a + na) and [b, b + nb) share a byte
bool stats_overlap(const void* a, u64 na, const void* b, u64 nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && (x < y ? y - x < na : x - y < nb);
}

// an output table lies in the bytes the call reads
bool stats_outputs_overlap(const void* src, u64 n, u64 count, const u32* d_hist, const u64* d_cost)
{
    return stats_overlap(src, n, d_hist, count * 256 * sizeof(u32)) || stats_overlap(src, n, d_cost, count * sizeof(u64));
}

// The launch for `nblocks` work entries of geometry G, the first `nlong` of them long (rcx_stats.hpp).  A workgroup holds
// 4 KiB of LDS and few registers: eight to a compute unit (32 waves, what a CU holds), and they loop over the units.
template <class G>
int stats_launch(rcx_ctx* c, const void* d_src, u64 n, u32 block, u64 nblocks, u64 nlong, u32* d_hist, u64* d_cost, hipStream_t s, G g)
{
    const u8* const src = static_cast<const u8*>(d_src);
    const u64 units = nlong + (nblocks - nlong + RCX_STATS_WAVES - 1) / RCX_STATS_WAVES, most = 8ull * (u64)c->cus;
    const u32 grid = (u32)(units < most ? units : most);
    hipLaunchKernelGGL(rcx_stats_k<G>, dim3(grid), dim3(RCX_STATS_THREADS), 0, s, src, n, block, nblocks, nlong, d_hist, d_cost, g);
    return LAUNCHED();
}

// the host-buffer calls behind the copy in: wait, then the tables back; the staging holds the counts, then the costs
int stats_host_finish(rcx_ctx* c, int launched, u64 count, u32* hist, u64* cost)
{
    if (launched != RCX_OK) return launched;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (hist) HIP_TRY(hipMemcpy(hist, c->h_out, count * 256 * sizeof(u32), hipMemcpyDeviceToHost));
    if (cost) HIP_TRY(hipMemcpy(cost, c->h_out + count * 256 * sizeof(u32), count * sizeof(u64), hipMemcpyDeviceToHost));
    return RCX_OK;
}

u32* stats_stage_hist(rcx_ctx* c, const u32* hist) { return hist ? reinterpret_cast<u32*>(c->h_out.get()) : nullptr; }
u64* stats_stage_cost(rcx_ctx* c, u64 count, const u64* cost) { return cost ? reinterpret_cast<u64*>(c->h_out.get() + count * 256 * sizeof(u32)) : nullptr; }

} // namespace

extern "C" {

int rcx_stats_blocks_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t block, uint32_t* d_hist, uint64_t* d_cost, void* stream)
{
    if (!c || !block_ok(block)) return RCX_E_ARG;
    const u64 nblocks = rcx_block_count(n, block);
    if (n && (!d_src || !(d_hist || d_cost) || stats_outputs_overlap(d_src, n, nblocks, d_hist, d_cost))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return stats_launch(c, d_src, n, block, nblocks, block > RCX_STATS_SHORT ? nblocks : 0, d_hist, d_cost, static_cast<hipStream_t>(stream), RcxBlocks{});
}

int rcx_stats_items_device(rcx_ctx* c, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* d_hist, uint64_t* d_cost,
                           void* stream)
{
    if (!c || (nitems && (!src_offsets || !(d_hist || d_cost)))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    ItemPlan& p = c->plan;
    int r = plan_crc_items(src_offsets, nitems, p);
    if (r != RCX_OK) return r;
    if (p.longest && !d_src) return RCX_E_ARG;
    if (d_src && stats_outputs_overlap(static_cast<const u8*>(d_src) + src_offsets[0], src_offsets[nitems] - src_offsets[0], nitems, d_hist, d_cost))
        return RCX_E_ARG;
    // the long entries lead the work order; in the caller's order (diagnostic) every entry is taken as long once one is
    u64 nlong = 0;
    if (items_sorted())
        while (nlong < p.nwork && p.len[nlong] > RCX_STATS_SHORT) ++nlong;
    else if (p.longest > RCX_STATS_SHORT)
        nlong = p.nwork;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    return stats_launch(c, d_src, 0, p.longest, p.nwork, nlong, d_hist, d_cost, s, g);
}

int rcx_stats_blocks(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t block, uint32_t* hist, uint64_t* cost)
{
    if (!c || !block_ok(block) || (n && (!src || !(hist || cost)))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const u64 nblocks = rcx_block_count(n, block);
    const int r = reserve_staging(c, n, nblocks * (256 * sizeof(u32) + sizeof(u64)), 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    return stats_host_finish(c, rcx_stats_blocks_device(c, c->h_in, n, block, stats_stage_hist(c, hist), stats_stage_cost(c, nblocks, cost), nullptr),
                             nblocks, hist, cost);
}

int rcx_stats_items(rcx_ctx* c, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* hist, uint64_t* cost)
{
    if (!c || (nitems && (!src_offsets || !(hist || cost)))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (nitems == 0) return RCX_OK;
    for (u64 i = 0; i < nitems; ++i)
        if (src_offsets[i + 1] < src_offsets[i] || src_offsets[i + 1] - src_offsets[i] > RCX_MAX_BLOCK) return RCX_E_ARG;
    const u64 base = src_offsets[0], n = src_offsets[nitems] - base;
    if (n && !src) return RCX_E_ARG;
    const int r = reserve_staging(c, n, nitems * (256 * sizeof(u32) + sizeof(u64)), 0);
    if (r != RCX_OK) return r;
    std::vector<u64> rel(nitems + 1); // the device copy begins at the first item
    for (u64 i = 0; i <= nitems; ++i) rel[i] = src_offsets[i] - base;
    if (n) HIP_TRY(hipMemcpy(c->h_in, src + base, n, hipMemcpyHostToDevice));
    return stats_host_finish(c, rcx_stats_items_device(c, c->h_in, rel.data(), nitems, stats_stage_hist(c, hist), stats_stage_cost(c, nitems, cost), nullptr),
                             nitems, hist, cost);
}

} // extern "C"
