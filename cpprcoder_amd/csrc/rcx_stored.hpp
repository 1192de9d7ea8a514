// rcx_stored.hpp -- stored blocks (include/rcx_stored.h): a block whose stream did not shrink is kept as its raw bytes.
// Two kernels, both for either call's use of them:
//
//   rcx_stored_sizes_k   mix, step 1: per block the rule of the header,
//                            stored[b] = coded_b + floor(len_b * gain / 65536) >= len_b      in uint64_t
//                        and the size of the block's mixed stream, len_b if stored, else coded_b.  An entry of the input
//                        table that decreases or points past comp_size is not followed: size 0, RCX_ST_CORRUPT at b.
//                        (Step 2 is rcx_scan_sizes_k as it is, rcx_kernels.hpp.)
//   rcx_stored_copy_k    the copy: entry e is `len` bytes from `from` to `to`, found on the device by the entry policy E --
//                        RcxMixEntries (mix, step 3: block b from d_src + b * block if stored, else from d_comp +
//                        offsets[b]) or RcxPickEntries (decode: the stored picks, whose stream must be as long as its output).
//
// The copy is shaped like rcx_stats_k (rcx_stats.hpp) on a fixed grid that loops over WORK UNITS: the first `nlong` entries
// are a unit each, copied by the whole workgroup; the others go four to a unit, one to a wave.  The host says where the
// short ones begin: with blocks all entries are of one kind (a block above RCX_COPY_SHORT bytes is long, and so are the
// short streams that were kept of such blocks: the workgroup copies any length); the picks are planned longest first.
// No wave waits for another: there is no barrier, no LDS, no inline assembly, no scratch.
//
// Both ends have any alignment, and their misalignment differs.  The bytes in front of the destination's first 16-byte
// border go one by one (at most 15), then 16 at a time -- loaded from a byte address (RcxU4AnyAlign, rcx_geom.hpp), stored
// aligned, RCX_COPY_ROWS loads a thread in flight -- then the rest one by one.  Nothing outside [from, from + len) is read
// and nothing outside [to, to + len) is written.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_geom.hpp"

#define RCX_COPY_WAVES 4
#define RCX_COPY_THREADS (64 * RCX_COPY_WAVES)
#define RCX_COPY_ROWS 4      // 16-byte loads a thread has in flight
#define RCX_COPY_SHORT 1024u // an entry of at most this many bytes is one wave's: a single row of 16-byte pieces

// the rule, in integers: gain is Q16, 0 .. 65535
RCX_HD bool rcx_is_stored(u64 coded, u64 len, u32 gain) { return coded + ((len * (u64)gain) >> 16) >= len; }

// [from, from + len) to [to, to + len) by `threads` threads of which this is thread t (threads >= 16)
__device__ __forceinline__ void rcx_copy_bytes(const u8* from, u8* to, u32 len, u32 t, u32 threads)
{
    u32 head = (u32)((0 - reinterpret_cast<uintptr_t>(to)) & 15u);
    if (head > len) head = len;
    if (t < head) to[t] = from[t];
    const u32 nvec = (len - head) >> 4;
    const RcxU4AnyAlign* q = reinterpret_cast<const RcxU4AnyAlign*>(from + head);
    U4* d = reinterpret_cast<U4*>(to + head);
    u32 v = t;
    for (; v + (RCX_COPY_ROWS - 1) * threads < nvec; v += RCX_COPY_ROWS * threads) {
        RcxU4AnyAlign x[RCX_COPY_ROWS];
#pragma unroll
        for (u32 j = 0; j < RCX_COPY_ROWS; ++j) x[j] = q[v + j * threads];
#pragma unroll
        for (u32 j = 0; j < RCX_COPY_ROWS; ++j) d[v + j * threads] = U4{x[j].x, x[j].y, x[j].z, x[j].w};
    }
    for (; v < nvec; v += threads) {
        const RcxU4AnyAlign x = q[v];
        d[v] = U4{x.x, x.y, x.z, x.w};
    }
    const u32 done = head + (nvec << 4);
    if (t < len - done) to[done + t] = from[done + t];
}

// Mix, step 3.  Entry b is block b: offsets[] is the mixed table (the scan's), stored[] the flags of step 1.  A stream that
// ends past dst_cap is not written (the scan has latched that); one of size 0 (a block whose input entry was not followed)
// copies nothing.
struct RcxMixEntries {
    const u8* src;
    u32 block;
    const u8* comp;
    const u64* comp_offsets;
    const u8* stored;
    const u64* offsets;
    u8* dst;
    u64 dst_cap;
    __device__ __forceinline__ bool find(u64 b, bool, const u8*& from, u8*& to, u32& len) const
    {
        const u64 o0 = offsets[b], o1 = offsets[b + 1];
        if (o1 > dst_cap || o1 == o0) return false;
        len = (u32)(o1 - o0); // at most the block's length
        from = stored[b] ? src + b * (u64)block : comp + comp_offsets[b];
        to = dst + o0;
        return true;
    }
};

// Decode.  Entry e is a stored pick in the tables of the item geometry: g.stream[e] names its stream, g.at[e] and g.len[e]
// its output, g.id[e] its position among the picks.  A stream that is not exactly as long as its output, or whose offsets
// are out of order or leave the buffer, is not copied: RCX_ST_CORRUPT with the pick position, flagged by `leader`.
struct RcxPickEntries {
    const u8* comp;
    u64 comp_size;
    const u64* comp_offsets;
    u8* dst;
    u32* status;
    RcxItems g;
    __device__ __forceinline__ bool find(u64 e, bool leader, const u8*& from, u8*& to, u32& len) const
    {
        const u64 st = g.stream[e];
        const u64 s0 = comp_offsets[st], s1 = comp_offsets[st + 1];
        len = g.len[e];
        if (!(s1 >= s0 && s1 <= comp_size && s1 - s0 == (u64)len)) {
            if (leader) rcx_flag(status, RCX_ST_CORRUPT, g.id[e]);
            return false;
        }
        from = comp + s0;
        to = dst + g.at[e];
        return true;
    }
};

// ===========================================================================
// Mix, step 1: sizes[b] and stored[b] of every block from the input table, one thread to a block on a grid that loops.
// ===========================================================================
__global__ __launch_bounds__(256) void rcx_stored_sizes_k(u64 n, u32 block, u64 nblocks, const u64* __restrict__ comp_offsets, u64 comp_size, u32 gain,
                                                          u32* __restrict__ sizes, u8* __restrict__ stored, u32* status)
{
    for (u64 b = (u64)blockIdx.x * 256u + threadIdx.x; b < nblocks; b += (u64)gridDim.x * 256u) {
        const u64 at = b * (u64)block;
        const u64 len = (n - at) < (u64)block ? (n - at) : (u64)block;
        const u64 s0 = comp_offsets[b], s1 = comp_offsets[b + 1];
        u32 size = 0;
        bool raw = false;
        if (s1 >= s0 && s1 <= comp_size) {
            raw = rcx_is_stored(s1 - s0, len, gain);
            size = (u32)(raw ? len : s1 - s0); // (kept: below len)
        } else {
            rcx_flag(status, RCX_ST_CORRUPT, b);
        }
        sizes[b] = size;
        stored[b] = raw ? 1 : 0;
    }
}

// ===========================================================================
// The copy.  Units 0 .. nlong - 1 are the entries of the same index, a workgroup to each; unit nlong + k is the entries
// nlong + 4k .. nlong + 4k + 3, a wave to each.
// ===========================================================================
template <class E>
__global__ __launch_bounds__(RCX_COPY_THREADS) void rcx_stored_copy_k(u64 nentries, u64 nlong, const E e)
{
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u64 units = nlong + (nentries - nlong + RCX_COPY_WAVES - 1) / RCX_COPY_WAVES;
    for (u64 unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const bool wide = unit < nlong; // (the same for every thread of the workgroup)
        const u64 ent = wide ? unit : nlong + (unit - nlong) * RCX_COPY_WAVES + wave;
        if (ent >= nentries) continue;
        const u8* from;
        u8* to;
        u32 len;
        if (!e.find(ent, (wide ? tid : lane) == 0, from, to, len)) continue;
        rcx_copy_bytes(from, to, len, wide ? tid : lane, wide ? (u32)RCX_COPY_THREADS : 64u);
    }
}
