// rcx_items.hpp -- the item calls of include/rcx.h: many independent buffers of differing sizes in one call, any
// subset of their streams back.  These calls instantiate the launch templates (rcx_launch.hpp: encode_launches /
// decode_launches) with the item geometry (rcx_geom.hpp, RcxItems).
//
// Everything that depends on the lengths is planned here, on the host, before anything is enqueued:
//   work order   entries sorted by length, longest first: a wave runs as long as its longest entry, so it should carry
//                entries of similar length, and the long chains should start first.  Items of length 0 get no entry.
//                RCX_ITEMS_ORDER=0 (diagnostic): the caller's order (within a length class, for encode).
//   classes      (encode) the scratch slot of an entry must hold the worst case of its length, and a wave addresses its
//                slots as base + lane * stride: entries are bucketed by the power of two at or above their length, one
//                launch per class with the stride of the class's upper bound -- at most twice what the entry needs.
//   tables       {offset, length, id, stream} per entry in work order and item -> entry for the size scan, one upload.
#pragma once

#include <algorithm>

#include "rcx_launch.hpp"

namespace
{

// the power of two at or above len, at least 16 and at most RCX_MAX_BLOCK: what a class's slots are sized for
u32 item_class_upper(u32 len)
{
    u32 up = 16;
    while (up < len) up <<= 1; // len <= RCX_MAX_BLOCK < 2^24
    return up > RCX_MAX_BLOCK ? RCX_MAX_BLOCK : up;
}

bool items_sorted() // RCX_ITEMS_ORDER=0 (diagnostic): keep the caller's order
{
    const char* v = getenv("RCX_ITEMS_ORDER");
    return !(v && atoi(v) == 0);
}

// Entry k of the call (an item, or a pick) has its bytes at table[k] .. table[k + 1] of the caller's buffer; for decode,
// pick[k] (or k) names its stream.  RCX_E_ARG for a table that is not monotonic, a length above RCX_MAX_BLOCK, a pick
// outside the set.
int plan_items(int coder, const u64* table, u64 count, const u64* pick, u64 nstreams, bool encode, ItemPlan& p)
{
    if (count > 0x7FFFFFFFull) return RCX_E_ARG;
    std::vector<u64> keys;
    keys.reserve(count);
    const bool sorted = items_sorted();
    for (u64 k = 0; k < count; ++k) {
        if (table[k + 1] < table[k] || table[k + 1] - table[k] > RCX_MAX_BLOCK) return RCX_E_ARG;
        if (!encode) {
            const u64 st = pick ? pick[k] : k;
            if (st >= nstreams) return RCX_E_ARG;
        }
        const u32 len = (u32)(table[k + 1] - table[k]);
        if (len == 0) continue;
        // ascending keys = descending length (or class only), then the caller's order
        const u32 rank = sorted ? len : (encode ? item_class_upper(len) : 0u);
        keys.push_back(((u64)(0xFFFFFFFFu - rank) << 32) | k);
    }
    if (sorted || encode) std::sort(keys.begin(), keys.end());
    const u64 nwork = keys.size();
    p.nwork = nwork;
    p.at.resize(nwork);
    p.len.resize(nwork);
    p.id.resize(nwork);
    p.stream.resize(encode ? 0 : nwork);
    p.inv.assign(encode ? count : 0, 0xFFFFFFFFu);
    p.classes.clear();
    p.slots_bytes = 0;
    p.longest = 0;
    for (u64 w = 0; w < nwork; ++w) {
        const u64 k = keys[w] & 0xFFFFFFFFull;
        const u32 len = (u32)(table[k + 1] - table[k]);
        p.at[w] = table[k];
        p.len[w] = len;
        p.id[w] = (u32)k;
        if (len > p.longest) p.longest = len;
        if (encode) {
            p.inv[k] = (u32)w;
            const u64 stride = rcx_block_bound_for(coder, item_class_upper(len));
            if (p.classes.empty() || p.classes.back().stride != stride) p.classes.push_back(ItemClass{w, 0, stride, p.slots_bytes});
            p.classes.back().count += 1;
            p.slots_bytes += stride;
        } else {
            p.stream[w] = (u32)(pick ? pick[k] : k);
        }
    }
    return RCX_OK;
}

// Device bytes a fresh context holds after an item call with this plan, the divisor tables apart (rcx_ctx_scratch_bytes).
u64 item_tables_bytes(const ItemPlan& p) { return p.nwork * (sizeof(u64) + 3 * sizeof(u32)) + p.inv.size() * sizeof(u32) + 16; }
u64 item_scratch_bytes(const ItemPlan& p, int coder, bool encode)
{
    if (p.nwork == 0) return 0;
    u64 b = item_tables_bytes(p) + (p.nwork + 1) * sizeof(u32); // tables, redo
    if (encode) {
        b += p.slots_bytes + 256 + (p.nwork + 1) * sizeof(u32); // slots, sizes
        if (is_rans(coder)) b += (p.nwork + 1) * sizeof(u32);   // starts
        if (coder == RCX_CODER_RANS) b += p.nwork * RCX_RANS_MODEL_DW * sizeof(u32);
    }
    return b;
}

// The tables go to the device in one copy: at[nwork] | len | id | stream | inv[items], the u64 part first.
int upload_items(rcx_ctx* c, const ItemPlan& p, hipStream_t s, RcxItems* g)
{
    const u64 bytes = item_tables_bytes(p);
    const int r = c->itab.reserve(bytes);
    if (r != RCX_OK) return r;
    c->itab_host.resize((bytes + 7) / 8);
    u8* h = reinterpret_cast<u8*>(c->itab_host.data());
    const u64 nw = p.nwork;
    u64 o = 0;
    auto put = [&](const void* from, u64 n) -> u64 {
        const u64 here = o;
        if (n) memcpy(h + o, from, n);
        o += n;
        return here;
    };
    const u64 o_at = put(p.at.data(), nw * sizeof(u64));
    const u64 o_len = put(p.len.data(), nw * sizeof(u32));
    const u64 o_id = put(p.id.data(), nw * sizeof(u32));
    const u64 o_stream = put(p.stream.data(), p.stream.size() * sizeof(u32));
    const u64 o_inv = put(p.inv.data(), p.inv.size() * sizeof(u32));
    // (a pageable source: the runtime has taken the bytes when the call returns, so the next call may refill itab_host)
    HIP_TRY(hipMemcpyAsync(c->itab, h, o, hipMemcpyHostToDevice, s));
    g->at = reinterpret_cast<const u64*>(c->itab + o_at);
    g->len = reinterpret_cast<const u32*>(c->itab + o_len);
    g->id = reinterpret_cast<const u32*>(c->itab + o_id);
    g->stream = reinterpret_cast<const u32*>(c->itab + o_stream);
    g->inv = reinterpret_cast<const u32*>(c->itab + o_inv);
    return RCX_OK;
}

RcxItems items_from(const RcxItems& g, u64 first) // the tables of a class: its entries begin `first` into the work order
{
    RcxItems r = g;
    r.at += first;
    r.len += first;
    r.id += first;
    r.stream += first;
    return r;
}

} // namespace

extern "C" {

uint64_t rcx_encode_items_bound(int coder, const uint64_t* src_offsets, uint64_t nitems)
{
    if (!src_offsets || !coder_ok(coder)) return 0;
    u64 total = 0;
    for (u64 i = 0; i < nitems; ++i) {
        const u64 len = src_offsets[i + 1] - src_offsets[i];
        if (src_offsets[i + 1] < src_offsets[i] || len > RCX_MAX_BLOCK) return 0;
        if (len) total += rcx_block_bound_for(coder, (u32)len);
    }
    return total;
}

int rcx_items_plan(int coder, const uint64_t* src_offsets, uint64_t nitems, uint32_t* work_order, uint64_t* nwork, uint64_t* scratch_bytes,
                   uint32_t* nclasses)
{
    if (!coder_ok(coder) || (nitems && !src_offsets)) return RCX_E_ARG;
    ItemPlan p;
    const int r = plan_items(coder, src_offsets, nitems, nullptr, 0, true, p);
    if (r != RCX_OK) return r;
    if (work_order)
        for (u64 w = 0; w < p.nwork; ++w) work_order[w] = p.id[w];
    if (nwork) *nwork = p.nwork;
    if (scratch_bytes) *scratch_bytes = item_scratch_bytes(p, coder, true);
    if (nclasses) *nclasses = (u32)p.classes.size();
    return RCX_OK;
}

int rcx_ctx_scratch_bytes(rcx_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return RCX_E_ARG;
    *bytes = c->slots.bytes() + c->sizes.bytes() + c->starts.bytes() + c->redo.bytes() + c->models.bytes() + c->itab.bytes();
    return RCX_OK;
}

int rcx_encode_items_device(rcx_ctx* c, int coder, const void* d_src, const uint64_t* src_offsets, uint64_t nitems,
                            void* d_dst, uint64_t dst_cap, uint64_t* d_comp_offsets, void* stream)
{
    if (!c || !coder_ok(coder) || !d_comp_offsets || (nitems && !src_offsets)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    ItemPlan& p = c->plan;
    int r = plan_items(coder, src_offsets, nitems, nullptr, 0, true, p);
    if (r != RCX_OK) return r;
    if (p.nwork == 0) return hipMemsetAsync(d_comp_offsets, 0, (nitems + 1) * sizeof(u64), s) == hipSuccess ? RCX_OK : RCX_E_HIP;
    if (!d_src || !d_dst) return RCX_E_ARG;
    // scratch: what the data asks for (at most twice its bound) and a fixed number of bytes per entry
    if ((r = reserve_scratch(c, coder, p.nwork, p.slots_bytes, p.longest)) != RCX_OK) return r;
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    // pass 1, a launch per class, the longest entries first; the launch shape follows the class's own count: a small
    // class of long entries is spread thin, not packed onto a few waves
    for (const ItemClass& k : p.classes) {
        ScratchView v{c->slots + k.slot_base, c->sizes + k.first, c->starts ? c->starts + k.first : nullptr,
                      c->models ? c->models + k.first * RCX_RANS_MODEL_DW : nullptr, c->redo + k.first};
        if ((r = encode_launches(c, coder, d_src, 0, p.longest, k.count, v, k.stride, s, false, items_from(g, k.first))) != RCX_OK) return r;
    }
    {
        Timed t(c, s, RCX_T_SCAN); // in the caller's order: offsets[i] = the sizes of the items before item i
        hipLaunchKernelGGL(rcx_scan_sizes_k<RcxItems>, dim3(1), dim3(1024), 0, s, c->sizes, nitems, d_comp_offsets, dst_cap, c->status, g);
    }
    {
        Timed t(c, s, RCX_T_SCATTER);
        for (const ItemClass& k : p.classes)
            hipLaunchKernelGGL(rcx_scatter_k<RcxItems>, dim3((u32)k.count), dim3(256), 0, s, c->slots + k.slot_base, k.stride, c->sizes + k.first,
                               d_comp_offsets, static_cast<u8*>(d_dst), dst_cap,
                               is_rans(coder) ? static_cast<const u32*>(c->starts + k.first) : static_cast<const u32*>(nullptr), items_from(g, k.first));
    }
    return LAUNCHED();
}

int rcx_decode_items_device(rcx_ctx* c, int coder, const void* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets,
                            uint64_t nstreams, const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, void* d_dst, void* stream)
{
    if (!c || !coder_ok(coder) || (npick && !dst_offsets) || nstreams > 0x7FFFFFFFull) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    ItemPlan& p = c->plan;
    int r = plan_items(coder, dst_offsets, npick, pick, nstreams, false, p);
    if (r != RCX_OK) return r;
    if (p.nwork == 0) return RCX_OK;
    if (!d_comp || !d_comp_offsets || !d_dst) return RCX_E_ARG;
    if (!is_rans(coder) && (r = ensure_divtab(c, p.longest)) != RCX_OK) return r;
    if ((r = ensure_redo(c, p.nwork)) != RCX_OK) return r;
    RcxItems g{};
    if ((r = upload_items(c, p, s, &g)) != RCX_OK) return r;
    // one launch for the whole work order (no slots, so no classes): the launch shape follows the call's entry count
    return decode_launches(c, coder, d_comp, comp_size, d_comp_offsets, p.nwork, p.longest, 0, d_dst, s, c->redo, false, g);
}

int rcx_encode_items(rcx_ctx* c, int coder, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems,
                     uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* comp_offsets)
{
    if (!c || !coder_ok(coder) || !dst_size || (nitems && !src_offsets)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    for (u64 i = 0; i < nitems; ++i)
        if (src_offsets[i + 1] < src_offsets[i] || src_offsets[i + 1] - src_offsets[i] > RCX_MAX_BLOCK) return RCX_E_ARG;
    const u64 base = nitems ? src_offsets[0] : 0, n = nitems ? src_offsets[nitems] - base : 0;
    if (n && (!src || !dst)) return RCX_E_ARG;
    const u64 bound = rcx_encode_items_bound(coder, src_offsets, nitems);
    int r = reserve_staging(c, n, bound, nitems + 1);
    if (r != RCX_OK) return r;
    std::vector<u64> rel(nitems + 1, 0); // the device copy begins at the first item
    for (u64 i = 0; i <= nitems && nitems; ++i) rel[i] = src_offsets[i] - base;
    if (n) HIP_TRY(hipMemcpy(c->h_in, src + base, n, hipMemcpyHostToDevice));
    if ((r = rcx_encode_items_device(c, coder, c->h_in, rel.data(), nitems, c->h_out, bound, c->h_off, nullptr)) != RCX_OK) return r;
    if ((r = rcx_ctx_sync_status(c, nullptr, nullptr)) != RCX_OK) return r;
    u64 total = 0;
    HIP_TRY(hipMemcpy(&total, c->h_off + nitems, sizeof(u64), hipMemcpyDeviceToHost));
    *dst_size = total;
    if (comp_offsets) HIP_TRY(hipMemcpy(comp_offsets, c->h_off, (nitems + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    if (total > dst_cap) return RCX_E_CAPACITY;
    if (total) HIP_TRY(hipMemcpy(dst, c->h_out, total, hipMemcpyDeviceToHost));
    return RCX_OK;
}

int rcx_decode_items(rcx_ctx* c, int coder, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets, uint64_t nstreams,
                     const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, uint8_t* dst, uint64_t dst_cap)
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
    std::vector<u64> rel(npick + 1);
    for (u64 k = 0; k <= npick; ++k) rel[k] = dst_offsets[k] - base;
    if (comp_size) HIP_TRY(hipMemcpy(c->h_in, comp, comp_size, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, comp_offsets, (nstreams + 1) * sizeof(u64), hipMemcpyHostToDevice));
    if ((r = rcx_decode_items_device(c, coder, c->h_in, comp_size, c->h_off, nstreams, pick, npick, rel.data(), c->h_out, nullptr)) != RCX_OK) return r;
    if ((r = rcx_ctx_sync_status(c, nullptr, nullptr)) != RCX_OK) return r;
    HIP_TRY(hipMemcpy(dst + base, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // extern "C"
