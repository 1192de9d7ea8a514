// rcx_picks_api.hpp -- the calls of include/rcx_picks.h on top of the planner of rcx_picks.hpp.
//
// rcx_decode_picks_device enqueues, and nothing else: the planner's four launches (the first clears its counters), the
// coder's decode launches with the counted item geometry (rcx_geom.hpp, RcxPicks: shaped by max_pick, the coded entries'
// count read by every wave) and, with flags, one launch of the copy kernel (rcx_stored.hpp) for the stored entries.  What
// depends on the tables' contents is decided on the device; what the host decides depends on max_pick and max_len alone.
//
// The scratch: the divisor table for max_len symbols (range coders), max_pick + 1 redo marks, and in the context's table
// scratch (which the host-planned item calls fill by upload)
//     at u64[max_pick] | len, id, stream u32[max_pick] | keys u32[max_pick] | cursor, bins u32[RCX_PICK_BINS] | counts u32[4]
#pragma once

#include "../../include/rcx_picks.h"
#include "rcx_picks.hpp"
#include "rcx_stored_api.hpp"

namespace
{

u64 picks_tables_bytes(u64 max_pick) { return max_pick * (sizeof(u64) + 4 * sizeof(u32)) + (2 * RCX_PICK_BINS + 4) * sizeof(u32); }

bool picks_sizes_ok(int coder, u64 max_pick, u32 max_len) { return coder_ok(coder) && max_pick <= 0x7FFFFFFFull && max_len <= RCX_MAX_BLOCK; }

int picks_reserve(rcx_ctx* c, int coder, u64 max_pick, u32 max_len)
{
    int r = is_rans(coder) ? RCX_OK : ensure_divtab(c, max_len);
    if (r == RCX_OK) r = ensure_redo(c, max_pick);
    return r == RCX_OK ? c->itab.reserve(picks_tables_bytes(max_pick)) : r;
}

RcxPickPlan picks_plan_in(u8* base, u64 max_pick)
{
    RcxPickPlan p;
    p.at = reinterpret_cast<u64*>(base);
    p.len = reinterpret_cast<u32*>(p.at + max_pick);
    p.id = p.len + max_pick;
    p.stream = p.id + max_pick;
    p.keys = p.stream + max_pick;
    p.cursor = p.keys + max_pick;
    p.bins = p.cursor + RCX_PICK_BINS;
    p.counts = p.bins + RCX_PICK_BINS;
    return p;
}

// workgroups of the planner's two entry kernels: one thread to an entry, eight workgroups to a compute unit at the most
u32 picks_grid(const rcx_ctx* c, u64 max_pick)
{
    const u64 want = (max_pick + RCX_PICK_THREADS - 1) / RCX_PICK_THREADS, most = 8ull * (u64)c->cus;
    return (u32)(want < most ? want : most);
}

} // namespace

extern "C" {

uint64_t rcx_picks_scratch_bytes(int coder, uint64_t max_pick, uint32_t max_len)
{
    if (!picks_sizes_ok(coder, max_pick, max_len) || max_pick == 0) return 0;
    return picks_tables_bytes(max_pick) + (max_pick + 1) * sizeof(u32);
}

int rcx_picks_reserve(rcx_ctx* c, int coder, uint64_t max_pick, uint32_t max_len)
{
    if (!c || !picks_sizes_ok(coder, max_pick, max_len)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_pick ? picks_reserve(c, coder, max_pick, max_len) : RCX_OK;
}

int rcx_decode_picks_device(rcx_ctx* c, int coder, const void* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets, uint64_t nstreams,
                            const uint8_t* d_stored, const uint64_t* d_pick, const uint64_t* d_dst_at, const uint64_t* d_dst_len,
                            const uint64_t* d_count, uint64_t max_pick, uint32_t max_len, void* d_dst, uint64_t dst_cap, void* stream)
{
    if (!c || !picks_sizes_ok(coder, max_pick, max_len) || nstreams > 0x7FFFFFFFull) return RCX_E_ARG;
    if (!d_comp || !d_comp_offsets || !d_pick || !d_dst_at || !d_dst_len || !d_count || !d_dst) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    if (max_pick == 0) return RCX_OK; // (a count above 0 is not seen: nothing is enqueued)
    int r = picks_reserve(c, coder, max_pick, max_len); // (after rcx_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    const RcxPickPlan p = picks_plan_in(c->itab, max_pick);
    const RcxPickTables t{d_pick, d_dst_at, d_dst_len, d_count, d_stored, d_comp_offsets, comp_size, nstreams, max_pick, dst_cap, max_len};
    const u32 grid = picks_grid(c, max_pick);
    hipLaunchKernelGGL(rcx_picks_clear_k, dim3(grid_for(RCX_PICK_BINS, RCX_PICK_THREADS)), dim3(RCX_PICK_THREADS), 0, s, p);
    hipLaunchKernelGGL(rcx_picks_classify_k, dim3(grid), dim3(RCX_PICK_THREADS), 0, s, t, p, c->status.get());
    hipLaunchKernelGGL(rcx_picks_scan_k, dim3(1), dim3(RCX_PICK_SCAN_THREADS), 0, s, p);
    hipLaunchKernelGGL(rcx_picks_scatter_k, dim3(grid), dim3(RCX_PICK_THREADS), 0, s, t, p);
    if ((r = LAUNCHED()) != RCX_OK) return r;
    RcxPicks g{};
    g.at = p.at;
    g.len = p.len;
    g.id = p.id;
    g.stream = p.stream;
    g.inv = nullptr;
    g.nlive = p.counts;
    // one launch for the whole work order, as the host-planned call has it; the launch shape follows max_pick
    if ((r = decode_launches(c, coder, d_comp, comp_size, d_comp_offsets, max_pick, max_len, 0, d_dst, s, c->redo, false, g)) != RCX_OK) return r;
    if (!d_stored) return RCX_OK;
    const RcxCountedPickEntries e{static_cast<const u8*>(d_comp), d_comp_offsets, static_cast<u8*>(d_dst), p.counts, max_pick, static_cast<const RcxItems&>(g)};
    hipLaunchKernelGGL(rcx_stored_copy_k<RcxCountedPickEntries>, dim3(stored_copy_grid(c, 2 * max_pick, max_pick)), dim3(RCX_COPY_THREADS), 0, s,
                       2 * max_pick, max_pick, e);
    return LAUNCHED();
}

int rcx_decode_picks(rcx_ctx* c, int coder, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets, uint64_t nstreams,
                     const uint8_t* stored, const uint64_t* pick, const uint64_t* dst_at, const uint64_t* dst_len, uint64_t npick, uint32_t max_len,
                     uint8_t* dst, uint64_t dst_cap)
{
    if (!c || !picks_sizes_ok(coder, npick, max_len) || nstreams > 0x7FFFFFFFull) return RCX_E_ARG;
    if (!comp || !comp_offsets || !dst || (npick && (!pick || !dst_at || !dst_len))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (npick == 0) return RCX_OK;
    // staging: the streams and the flags in h_in; the stream table, the three pick tables and the count in h_off; dst in h_out
    const u64 flags_at = (comp_size + 15) & ~15ull;
    int r = reserve_staging(c, flags_at + nstreams, dst_cap, nstreams + 1 + 3 * npick + 1);
    if (r != RCX_OK) return r;
    u64* const d_pick = c->h_off + nstreams + 1;
    u64* const d_at = d_pick + npick;
    u64* const d_len = d_at + npick;
    u64* const d_count = d_len + npick;
    u8* const d_flags = c->h_in + flags_at;
    if (comp_size) HIP_TRY(hipMemcpy(c->h_in, comp, comp_size, hipMemcpyHostToDevice));
    if (stored && nstreams) HIP_TRY(hipMemcpy(d_flags, stored, nstreams, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, comp_offsets, (nstreams + 1) * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pick, pick, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_at, dst_at, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, dst_len, npick * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, &npick, sizeof(u64), hipMemcpyHostToDevice));
    if (dst_cap) HIP_TRY(hipMemcpy(c->h_out, dst, dst_cap, hipMemcpyHostToDevice)); // (what no pick writes stays as it is)
    r = rcx_decode_picks_device(c, coder, c->h_in, comp_size, c->h_off, nstreams, stored ? d_flags : nullptr, d_pick, d_at, d_len, d_count, npick, max_len,
                                c->h_out, dst_cap, nullptr);
    if (r != RCX_OK) return r;
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (dst_cap) HIP_TRY(hipMemcpy(dst, c->h_out, dst_cap, hipMemcpyDeviceToHost)); // (the good entries also behind a latched failure)
    return r;
}

} // extern "C"
