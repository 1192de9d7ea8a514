// rcx_stored_items.hpp -- stored items (include/rcx_stored_items.h): the mix of rcx_stored.hpp with the items of an item
// encode call as its entries.  An item whose stream did not shrink is kept as its raw bytes.
//
//   rcx_stored_item_sizes_k   mix, step 1: per item, in the caller's order, the rule of rcx_stored.h (rcx_is_stored as it is)
//                             and the size of the item's mixed stream, len_i if stored, else coded_i.  The length comes from
//                             the uploaded tables (RcxItems: item -> work entry -> length); an item of length 0 has no entry,
//                             no stream, and is never stored.  An entry of the input table that decreases or points past
//                             comp_size is not followed: size 0, RCX_ST_CORRUPT at the item.  The sizes go to the context's
//                             size table in WORK order, where rcx_scan_sizes_k<RcxItems> (step 2, as it is) looks for them;
//                             the flags are in the caller's order.
//   RcxMixItemEntries         mix, step 3: the entry policy of a third instance of rcx_stored_copy_k.  Entry e of the work
//                             order is item g.id[e]: from d_src + g.at[e] if stored, else from d_comp + comp_offsets[item],
//                             to d_dst + offsets[item].
//
// Unlike blocks the entries are of both kinds in one call: the host plans them longest first by ITEM length, the entries
// above RCX_COPY_SHORT bytes are the `nlong` workgroup entries, the rest go four to a unit.  A short stream that was kept of
// a long item is copied by a workgroup, as with blocks; a kept stream of a short item is shorter still.
// As in rcx_stored.hpp: no barrier, no LDS, no inline assembly, no scratch, no wave that waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_stored.hpp"

struct RcxMixItemEntries {
    const u8* src;
    const u8* comp;
    const u64* comp_offsets;
    const u8* stored;
    const u64* offsets;
    u8* dst;
    u64 dst_cap;
    RcxItems g;
    __device__ __forceinline__ bool find(u64 e, bool, const u8*& from, u8*& to, u32& len) const
    {
        const u64 item = g.id[e];
        const u64 o0 = offsets[item], o1 = offsets[item + 1];
        if (o1 > dst_cap || o1 == o0) return false; // (latched by the scan; an item whose input entry was not followed)
        len = (u32)(o1 - o0); // at most the item's length
        from = stored[item] ? src + g.at[e] : comp + comp_offsets[item];
        to = dst + o0;
        return true;
    }
};

// ===========================================================================
// Mix, step 1: one thread to an item on a grid that loops.  sizes[] has an entry per work entry; the scan reads it
// through g.inv, and takes 0 for an item without one.
// ===========================================================================
__global__ __launch_bounds__(256) void rcx_stored_item_sizes_k(u64 nitems, const u64* __restrict__ comp_offsets, u64 comp_size, u32 gain,
                                                               u32* __restrict__ sizes, u8* __restrict__ stored, u32* status, const RcxItems g)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < nitems; i += (u64)gridDim.x * 256u) {
        const u32 w = g.inv[i];
        bool raw = false;
        if (w != 0xFFFFFFFFu) {
            const u64 len = g.len[w];
            const u64 s0 = comp_offsets[i], s1 = comp_offsets[i + 1];
            u32 size = 0;
            if (s1 >= s0 && s1 <= comp_size) {
                raw = rcx_is_stored(s1 - s0, len, gain);
                size = (u32)(raw ? len : s1 - s0); // (kept: below len)
            } else {
                rcx_flag(status, RCX_ST_CORRUPT, i);
            }
            sizes[w] = size;
        }
        stored[i] = raw ? 1 : 0;
    }
}
