// rcx_geom.hpp -- where a coding kernel finds the bytes of its work entry `blk`: the geometry policy.
//
// Every coding kernel is a template over one of these two.  RcxBlocks is the many-block geometry (one buffer cut into
// blocks of one size: position and length follow from the index); it is empty, and a kernel instantiated with it is
// the kernel the block calls always ran.  RcxItems is the item geometry (rcx_encode_items* / rcx_decode_items*,
// include/rcx.h): position and length come from tables in WORK ORDER that the host planned (rcx_api.hip, ItemPlan) and
// uploaded with the call.  A launch covers the entries of one length class, whose scratch slots share a stride: the
// table pointers, like sizes / redo / starts / models, are already advanced to the class's first entry, so a kernel
// indexes all of them by `blk` as before.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_lane.hpp"

struct RcxBlocks {
    static constexpr bool items = false;
};

struct RcxItems {
    static constexpr bool items = true;
    const u64* at;     // byte offset of the entry's bytes in d_src (encode) / d_dst (decode)
    const u32* len;    // its length, 1 .. RCX_MAX_BLOCK (an item of length 0 has no entry)
    const u32* id;     // what a failure reports: the item (encode, also its place in the offsets table), the pick position (decode)
    const u32* stream; // decode: which stream of the compacted set the entry reads
    const u32* inv;    // the size scan, which runs in the caller's order: item -> its work entry, 0xFFFFFFFF for an item of length 0
};

// The block geometry's two lines stay in the kernels as they were (at = blk * block, len = min(block, n - at)); the
// item geometry replaces their result with the tables' (and leaves them without a use).  A lane without an entry has
// length 0 and the position of the launch's first entry -- its longest: where a kernel lets such a lane read along with
// the others, it reads bytes that are there.
__device__ __forceinline__ void rcx_where(const RcxItems& g, bool live, u64 blk, u64& at, u32& len)
{
    at = g.at[live ? blk : 0];
    len = live ? g.len[blk] : 0u;
}

// the index a latched failure names
__device__ __forceinline__ u64 rcx_id(const RcxBlocks&, u64 blk) { return blk; }
__device__ __forceinline__ u64 rcx_id(const RcxItems& g, u64 blk) { return g.id[blk]; }
// the entry's place in the table of compacted streams (decode)
__device__ __forceinline__ u64 rcx_stream_of(const RcxBlocks&, u64 blk) { return blk; }
__device__ __forceinline__ u64 rcx_stream_of(const RcxItems& g, u64 blk) { return g.stream[blk]; }

// stream size of entry b of the offsets table (the scan): sizes[] is in work order
__device__ __forceinline__ u32 rcx_size_of(const RcxBlocks&, const u32* sizes, u64 b) { return sizes[b]; }
__device__ __forceinline__ u32 rcx_size_of(const RcxItems& g, const u32* sizes, u64 b)
{
    const u32 w = g.inv[b];
    return w == 0xFFFFFFFFu ? 0u : sizes[w];
}

// 16 decoded bytes to an output of any alignment (the item geometry: an item begins where the one before it ends).
// gfx950 serves a global 16-byte store at any byte address; what a misaligned one costs is once per 16 symbols and
// off the symbol chain (tools/items_rate.py, part B, measures it).
struct __attribute__((packed, aligned(1))) RcxU4AnyAlign {
    u32 x, y, z, w;
};
template <bool ANY_ALIGN>
__device__ __forceinline__ void rcx_store16(u8* p, const U4& v)
{
    if (ANY_ALIGN) *reinterpret_cast<RcxU4AnyAlign*>(p) = RcxU4AnyAlign{v.x, v.y, v.z, v.w};
    else *reinterpret_cast<U4*>(p) = v;
}
