// rcx_geom.hpp -- where a coding kernel finds the bytes of its work entry `blk`: the geometry policy.
//
// Every coding kernel is a template over one of these.  RcxBlocks is the many-block geometry (one buffer cut into
// blocks of one size: position and length follow from the index); it is empty, and a kernel instantiated with it is
// the kernel the block calls always ran.  RcxItems is the item geometry (rcx_encode_items* / rcx_decode_items*,
// include/rcx.h): position and length come from tables in WORK ORDER that the host planned (rcx_api.hip, ItemPlan) and
// uploaded with the call.  A launch covers the entries of one length class, whose scratch slots share a stride: the
// table pointers, like sizes / redo / starts / models, are already advanced to the class's first entry, so a kernel
// indexes all of them by `blk` as before.  RcxPicks (rcx_decode_picks_device, include/rcx_picks.h) is the item geometry
// whose tables a kernel planned (rcx_picks.hpp): the launch is shaped by the most entries there can be, and how many of the
// tables' entries are meant is a word in device memory that every wave reads when it opens (`counted`).  RcxEncPicks
// (rcx_encode_picks_device, include/rcx_encode_picks.h) is the counted geometry of the encoders (`planned`): the work order
// is laid out in UNITS of 64 entries, every length class begins a unit, and the stride and the base of the scratch slots
// are the unit's -- one launch covers all classes, and its shape follows the most entries there can be.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_lane.hpp"

struct RcxBlocks {
    static constexpr bool items = false;
    static constexpr bool counted = false;
    static constexpr bool planned = false;
};

struct RcxItems {
    static constexpr bool items = true;
    static constexpr bool counted = false;
    static constexpr bool planned = false;
    const u64* at;     // byte offset of the entry's bytes in d_src (encode) / d_dst (decode)
    const u32* len;    // its length, 1 .. RCX_MAX_BLOCK (an item of length 0 has no entry)
    const u32* id;     // what a failure reports: the item (encode, also its place in the offsets table), the pick position (decode)
    const u32* stream; // decode: which stream of the compacted set the entry reads
    const u32* inv;    // the size scan, which runs in the caller's order: item -> its work entry, 0xFFFFFFFF for an item of length 0
};

// The decoders only.  Entries 0 .. *nlive - 1 of the tables are meant; what lies behind them is never read (entry 0 apart,
// as above, so the tables have one entry at least).
struct RcxPicks : RcxItems {
    static constexpr bool counted = true;
    const u32* nlive;
};

// The encoders only.  Work entries 0 .. *nlive - 1 are laid out (a multiple of 64); an entry of length 0 among them is a
// HOLE, the padding behind a class's last entry: it is not live and has no slot.  Entries 64 u .. 64 u + 63 have their
// slots at slots + unit[u].base + (entry & 63) * unit[u].stride.  Every encoder's group of entries (a workgroup's
// lanes_used, a wave's 64, an octet wave's 8) divides 64 and begins on a multiple of itself, so a group lies in one unit
// and its stride is wave-uniform.
struct RcxEncUnit {
    u64 base;   // bytes into the slots
    u32 stride; // rcx_block_bound_for(coder, the class's upper length)
    u32 spare;
};
struct RcxEncPicks : RcxItems {
    static constexpr bool counted = true;
    static constexpr bool planned = true;
    const u32* nlive;
    const RcxEncUnit* unit;
};

// Where entry `blk` lies.  A lane without an entry has length 0 and the position of the launch's first entry -- with
// items its longest: where a kernel lets such a lane read along with the others, it reads bytes that are there.
__device__ __forceinline__ void rcx_where(const RcxItems& g, bool live, u64 blk, u64& at, u32& len)
{
    at = g.at[live ? blk : 0];
    len = live ? g.len[blk] : 0u;
}

// How every coding kernel opens.  RCX_ENTRY declares `live` (the lane has an entry), `at` and `len` for work entry BLK
// of geometry GEOM: with blocks, position and length follow from the index (the last block of a buffer is the short
// one); with items they are the tables' (and the block lines are left without a use).  RCX_ENTRY_ONLY is the same for a
// kernel that can run as the second pass behind a many-lane kernel: ONLY != nullptr leaves just the entries that one
// marked (ONLY[blk] != 0), and a wave none of whose lanes has an entry returns.
// With a counted geometry (RcxPicks) `live` also asks the device's count, and a wave none of whose lanes has an entry
// returns: the launch is shaped for the most entries there can be, and no decoder has a barrier.  (`if constexpr` on a
// dependent condition: the other geometries' kernels are instantiated without these lines.)  With a planned geometry
// (RcxEncPicks) a hole is not live either; the multi-wave encoders have barriers, but every wave of their workgroups
// carries the same entries, so the workgroup returns as a whole or not at all.
// Macros, not functions: a function is optimised on its own before it is inlined into the kernel, and what arrives
// there differs enough from these lines written in place that 18 of the 50 kernels came out with different
// instructions, down into their symbol loops (tools/diag/kernel_diff.py).
#define RCX_ENTRY_COUNTED(GEOM, BLK)                                                                  \
    if constexpr (decltype(GEOM)::counted) {                                                          \
        live = live && (BLK) < (u64)(GEOM).nlive[0];                                                  \
        if (!__any(live)) return;                                                                     \
    }                                                                                                 \
    if constexpr (decltype(GEOM)::planned) {                                                          \
        live = live && (GEOM).len[BLK] != 0;                                                          \
        if (!__any(live)) return;                                                                     \
    }
#define RCX_ENTRY_WHERE(GEOM, BLK, N, BLOCK)                                                          \
    u64 at = live ? (BLK) * (u64)(BLOCK) : 0;                                                         \
    u32 len = live ? (u32)(((N) - at) < (u64)(BLOCK) ? ((N) - at) : (u64)(BLOCK)) : 0u;               \
    if constexpr (decltype(GEOM)::items) rcx_where(GEOM, live, BLK, at, len)
#define RCX_ENTRY(GEOM, BLK, NBLOCKS, N, BLOCK)                                                       \
    bool live = (BLK) < (NBLOCKS);                                                                    \
    RCX_ENTRY_COUNTED(GEOM, BLK)                                                                      \
    RCX_ENTRY_WHERE(GEOM, BLK, N, BLOCK)
#define RCX_ENTRY_ONLY(GEOM, BLK, NBLOCKS, N, BLOCK, ONLY)                                            \
    bool live = (BLK) < (NBLOCKS);                                                                    \
    RCX_ENTRY_COUNTED(GEOM, BLK)                                                                      \
    if (ONLY) {                                                                                       \
        live = live && (ONLY)[BLK] != 0;                                                              \
        if (!__any(live)) return;                                                                     \
    }                                                                                                 \
    RCX_ENTRY_WHERE(GEOM, BLK, N, BLOCK)

// Behind RCX_ENTRY in an encoder: with a planned geometry the kernel's SLOTS and SLOT (its parameters, which it goes on
// to use as slots + entry * slot) become those of the unit of the wave's first lane, whose entry the launch always has.
#define RCX_ENTRY_SLOTS(GEOM, BLK, SLOTS, SLOT)                                                       \
    if constexpr (decltype(GEOM)::planned) {                                                          \
        const u32 unit_ = __builtin_amdgcn_readfirstlane((u32)((BLK) >> 6));                          \
        SLOT = (GEOM).unit[unit_].stride;                                                             \
        SLOTS += (GEOM).unit[unit_].base - (u64)unit_ * 64u * (SLOT);                                 \
    }

// The fast paths' condition (16 bytes at a go, no per-symbol length test), behind RCX_ENTRY: every lane of the wave has
// a whole block, blocks are multiples of 16 bytes and P, the buffer the blocks lie in, is 16-byte aligned.  Never with
// items, which begin where the one before ends.  (A macro for RCX_ENTRY's reason: as a function it changed three kernels.)
#define RCX_ALL_FULL(GEOM, BLOCK, P)                                                                  \
    (!decltype(GEOM)::items && __all(live && len == (BLOCK)) && ((BLOCK) % 16u == 0) && ((reinterpret_cast<uintptr_t>(P) & 15u) == 0))

// the index a latched failure names
__device__ __forceinline__ u64 rcx_id(const RcxBlocks&, u64 blk) { return blk; }
__device__ __forceinline__ u64 rcx_id(const RcxItems& g, u64 blk) { return g.id[blk]; }
// the entry's place in the table of compacted streams (decode)
__device__ __forceinline__ u64 rcx_stream_of(const RcxBlocks&, u64 blk) { return blk; }
__device__ __forceinline__ u64 rcx_stream_of(const RcxItems& g, u64 blk) { return g.stream[blk]; }

// The entry's stream in the compacted set, for a decoder (behind RCX_ENTRY, for its reason macros): RCX_STREAM declares
// s0, s1 -- where it begins and ends in the compressed buffer -- and sets stream_len; RCX_STREAM_OK: the two offsets are
// in order, inside the buffer, and at least MIN bytes apart.  (An offset table that points past the buffer is not followed.)
#define RCX_STREAM(GEOM, BLK, OFFSETS)                                                                \
    const u64 sidx = rcx_stream_of(GEOM, BLK);                                                        \
    const u64 s0 = (OFFSETS)[sidx], s1 = (OFFSETS)[sidx + 1];                                         \
    stream_len = s1 - s0
#define RCX_STREAM_OK(COMP_SIZE, MIN) (s1 >= s0 && s1 <= (COMP_SIZE) && stream_len >= (MIN))

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
