// rcx_encode_picks_api.hpp -- the calls of include/rcx_encode_picks.h on top of the planner of rcx_encode_picks.hpp.
//
// rcx_encode_picks_device enqueues, and nothing else: the planner's four launches (the first clears its counters), the
// coder's encode launches with the planned item geometry (rcx_geom.hpp, RcxEncPicks: ONE launch of every kernel for all
// length classes, shaped by max_items, the stride and the base of the slots read per unit of 64 entries), the size scan
// and the scatter.  What depends on the tables' contents is decided on the device; what the host decides -- the static
// coder's choice between its kernels, the entries per multi-wave workgroup -- depends on max_items alone.
//
// The scratch (the formula is in the header): slots, sizes, redo, starts and models as the host-planned call has them,
// for P = max_items + RCX_EPICK_PAD work positions, and in the context's table scratch
//     at u64[P] | total u64[2] | unit (4 P bytes: 16 per 64 positions, + 1) | len, id u32[P] | inv, keys u32[max_items] |
//     cursor, bins u32[RCX_EPICK_BINS] | counts u32[4]
#pragma once

#include "../../include/rcx_encode_picks.h"
#include "rcx_encode_picks.hpp"
#include "rcx_items.hpp"
#include "rcx_picks_api.hpp"

namespace
{

u64 epicks_positions(u64 max_items) { return max_items + RCX_EPICK_PAD; }
// the launches' entry count: every class padded to a unit at the most, rounded up to a unit
u64 epicks_launch_entries(u64 max_items) { return ((max_items + 63) & ~63ull) + 64ull * RCX_EPICK_CLASSES; }

u64 epicks_tables_bytes(u64 max_items)
{
    const u64 P = epicks_positions(max_items);
    return P * (sizeof(u64) + 3 * sizeof(u32)) + 2 * sizeof(u64) + max_items * 2 * sizeof(u32) + (2 * RCX_EPICK_BINS + 4) * sizeof(u32);
}

// what the slots of entries of max_bytes bytes between them can take, each in the class of its own length
u64 epicks_slots_bytes(int coder, u64 max_items, u64 max_bytes)
{
    return is_rans(coder) ? 4 * max_bytes + 1152 * max_items : 3 * max_bytes + 2112 * max_items;
}

bool epicks_sizes_ok(int coder, u64 max_items, u32 max_len) { return coder_ok(coder) && max_items <= 0x7FFFFFFFull && max_len <= RCX_MAX_BLOCK; }

RcxEpickPlan epicks_plan_in(u8* base, u64 max_items)
{
    const u64 P = epicks_positions(max_items);
    RcxEpickPlan p;
    p.at = reinterpret_cast<u64*>(base);
    p.total = p.at + P;
    p.unit = reinterpret_cast<RcxEncUnit*>(p.total + 2);
    p.len = reinterpret_cast<u32*>(p.unit) + P;
    p.id = p.len + P;
    p.inv = p.id + P;
    p.keys = p.inv + max_items;
    p.cursor = p.keys + max_items;
    p.bins = p.cursor + RCX_EPICK_BINS;
    p.counts = p.bins + RCX_EPICK_BINS;
    return p;
}

RcxEpickClasses epicks_classes(int coder)
{
    RcxEpickClasses cl;
    for (u32 k = 0; k < RCX_EPICK_CLASSES; ++k) {
        cl.first_bin[k] = rcx_epick_bin(rcx_epick_upper(k));
        cl.stride[k] = (u32)rcx_block_bound_for(coder, rcx_epick_upper(k));
    }
    cl.first_bin[RCX_EPICK_CLASSES] = RCX_EPICK_BINS;
    return cl;
}

// Everything a call needs that is not a launch on its stream: memory, the divisor table, a kernel's leave for dynamic LDS.
int epicks_reserve(rcx_ctx* c, int coder, u64 max_items, u32 max_len, u64 max_bytes)
{
    const u64 P = epicks_positions(max_items);
    int r = reserve_scratch(c, coder, P, epicks_slots_bytes(coder, max_items, max_bytes), max_len);
    if (r == RCX_OK) r = c->itab.reserve(epicks_tables_bytes(max_items));
    // (as encode_launches asks, so that it finds both done: the two-wave kernel, and the one-wave kernel of RCX_RANS1_WAVES=1)
    if (r == RCX_OK && coder == RCX_CODER_RANS) r = allow_lds(c, &rcx_enc_rans1w_k<RcxEncPicks>, RCX_R1W_LDS_BYTES);
    if (r == RCX_OK && coder == RCX_CODER_RANS) r = allow_lds(c, &rcx_enc_rans1_k<RcxEncPicks>, 128 * 1024);
    return r;
}

} // namespace

extern "C" {

uint64_t rcx_encode_picks_scratch_bytes(int coder, uint64_t max_items, uint32_t max_len, uint64_t max_bytes)
{
    if (!epicks_sizes_ok(coder, max_items, max_len) || max_items == 0) return 0;
    const u64 P = epicks_positions(max_items);
    u64 b = epicks_tables_bytes(max_items) + epicks_slots_bytes(coder, max_items, max_bytes) + 256 + 2 * (P + 1) * sizeof(u32);
    if (is_rans(coder)) b += (P + 1) * sizeof(u32);
    if (coder == RCX_CODER_RANS) b += P * RCX_RANS_MODEL_DW * sizeof(u32);
    return b;
}

int rcx_encode_picks_reserve(rcx_ctx* c, int coder, uint64_t max_items, uint32_t max_len, uint64_t max_bytes)
{
    if (!c || !epicks_sizes_ok(coder, max_items, max_len)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return max_items ? epicks_reserve(c, coder, max_items, max_len, max_bytes) : RCX_OK;
}

int rcx_encode_picks_device(rcx_ctx* c, int coder, const void* d_src, uint64_t src_cap, const uint64_t* d_src_at, const uint64_t* d_src_len,
                            const uint64_t* d_count, uint64_t max_items, uint32_t max_len, uint64_t max_bytes, void* d_dst, uint64_t dst_cap,
                            uint64_t* d_comp_offsets, void* stream)
{
    if (!c || !epicks_sizes_ok(coder, max_items, max_len)) return RCX_E_ARG;
    if (!d_src || !d_src_at || !d_src_len || !d_count || !d_dst || !d_comp_offsets) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    if (max_items == 0) return RCX_OK; // (a count above 0 is not seen: nothing is enqueued)
    int r = epicks_reserve(c, coder, max_items, max_len, max_bytes); // (after rcx_encode_picks_reserve: nothing to do)
    if (r != RCX_OK) return r;
    const u64 P = epicks_positions(max_items), entries = epicks_launch_entries(max_items);
    const RcxEpickPlan p = epicks_plan_in(c->itab, max_items);
    const RcxEpickTables t{d_src_at, d_src_len, d_count, src_cap, max_items, max_bytes, P, max_len};
    const u32 grid = picks_grid(c, max_items);
    hipLaunchKernelGGL(rcx_epicks_clear_k, dim3(grid_for(RCX_EPICK_BINS, RCX_PICK_THREADS)), dim3(RCX_PICK_THREADS), 0, s, p);
    hipLaunchKernelGGL(rcx_epicks_classify_k, dim3(grid), dim3(RCX_PICK_THREADS), 0, s, t, p, c->status.get());
    hipLaunchKernelGGL(rcx_epicks_scan_k, dim3(1), dim3(RCX_PICK_SCAN_THREADS), 0, s, t, p, epicks_classes(coder), c->status.get());
    hipLaunchKernelGGL(rcx_epicks_scatter_k, dim3(grid), dim3(RCX_PICK_THREADS), 0, s, t, p);
    if ((r = LAUNCHED()) != RCX_OK) return r;
    RcxEncPicks g{};
    g.at = p.at;
    g.len = p.len;
    g.id = p.id;
    g.stream = nullptr;
    g.inv = p.inv;
    g.nlive = p.counts;
    g.unit = p.unit;
    // pass 1, one launch of every kernel for all classes; `slot` is a unit's own, the one given here is not used
    const ScratchView v{c->slots, c->sizes, c->starts, c->models, c->redo};
    if ((r = encode_launches(c, coder, d_src, 0, max_len, entries, v, 0, s, false, g)) != RCX_OK) return r;
    {
        Timed tm(c, s, RCX_T_SCAN);
        hipLaunchKernelGGL(rcx_epicks_sizes_k, dim3(1), dim3(1024), 0, s, c->sizes.get(), d_count, max_items, d_comp_offsets, dst_cap, c->status.get(), g);
    }
    {
        Timed tm(c, s, RCX_T_SCATTER);
        hipLaunchKernelGGL(rcx_scatter_k<RcxEncPicks>, dim3((u32)entries), dim3(256), 0, s, c->slots.get(), (u64)0, c->sizes.get(), d_comp_offsets,
                           static_cast<u8*>(d_dst), dst_cap, is_rans(coder) ? static_cast<const u32*>(c->starts) : static_cast<const u32*>(nullptr), g);
    }
    return LAUNCHED();
}

int rcx_encode_picks(rcx_ctx* c, int coder, const uint8_t* src, uint64_t src_cap, const uint64_t* src_at, const uint64_t* src_len, uint64_t nitems,
                     uint32_t max_len, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* comp_offsets)
{
    if (!c || !epicks_sizes_ok(coder, nitems, max_len) || !dst_size) return RCX_E_ARG;
    if (!src || !dst || (nitems && (!src_at || !src_len))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    if (nitems == 0) {
        if (comp_offsets) comp_offsets[0] = 0;
        return RCX_OK;
    }
    u64 max_bytes = 0; // the valid entries', by the device's rules
    for (u64 k = 0; k < nitems; ++k)
        if (src_len[k] <= max_len && src_at[k] <= src_cap && src_len[k] <= src_cap - src_at[k]) max_bytes += src_len[k];
    // staging: the source in h_in; the two tables, the count and the offsets in h_off; the streams in h_out
    int r = reserve_staging(c, src_cap, dst_cap, 2 * nitems + 1 + nitems + 1);
    if (r != RCX_OK) return r;
    u64* const d_at = c->h_off;
    u64* const d_len = d_at + nitems;
    u64* const d_count = d_len + nitems;
    u64* const d_offs = d_count + 1;
    if (src_cap) HIP_TRY(hipMemcpy(c->h_in, src, src_cap, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_at, src_at, nitems * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, src_len, nitems * sizeof(u64), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, &nitems, sizeof(u64), hipMemcpyHostToDevice));
    r = rcx_encode_picks_device(c, coder, c->h_in, src_cap, d_at, d_len, d_count, nitems, max_len, max_bytes, c->h_out, dst_cap, d_offs, nullptr);
    if (r != RCX_OK) return r;
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    u64 total = 0;
    HIP_TRY(hipMemcpy(&total, d_offs + nitems, sizeof(u64), hipMemcpyDeviceToHost));
    *dst_size = total;
    if (comp_offsets) HIP_TRY(hipMemcpy(comp_offsets, d_offs, (nitems + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    const u64 back = total < dst_cap ? total : dst_cap;
    if (back) HIP_TRY(hipMemcpy(dst, c->h_out, back, hipMemcpyDeviceToHost)); // (the good entries also behind a latched failure)
    return r;
}

} // extern "C"
