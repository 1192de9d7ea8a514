// rcx_kernels.hpp -- the gfx950 kernels of the library: what all of them share, the two kernels behind every
// encoder's pass 1, and the include list of the kernel families in dependency order.
//
//   RCX_ST_*, rcx_flag   how a kernel reports a failure
//   rcx_wave_max, rcx_byte_of
//   rcx_scan_sizes_k     size prefix: exclusive scan of sizes[] -> offsets[] (u64)
//   rcx_scatter_k        pass 2: compacted scatter of the slots to dst + offsets[b]
//                        (the reference's MemoryStream is the sink, cpprcoder.h:1031-1054)
//
//   rcx_adaptive.hpp     the adaptive range coder, one lane per block, and its resumable forms
//   rcx_quad.hpp         the "4 lanes per block" decoders' frame + the adaptive one
//   rcx_mc.hpp           the multi-wave range encoders' machinery + the adaptive one
//   rcx_static.hpp, rcx_rans.hpp, rcx_bwt.hpp   the static range coder, the rANS coders, the block sort
//   rcx_crc.hpp          CRC-32 per block or item, stored or verified
//   rcx_stats.hpp        byte counts and order-0 cost per block or item
//   rcx_planes.hpp       the byte-plane filter for typed data, split and join
//   rcx_stored.hpp       stored blocks: the rule per block, and the copy of raw and kept streams
//
// Roofline class: HBM-bound integer/byte work, no MFMA.  What actually bounds the
// coder kernels is the serial dependency chain of one symbol (divide -> multiply ->
// renormalise -> table update) times the number of blocks in flight; see DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_lane.hpp"
#include "rcx_geom.hpp"

#define RCX_ST_CAPACITY 1u
#define RCX_ST_CORRUPT 2u

// status[0] = OR of RCX_ST_* flags, status[1] = lowest failing block (saturated to u32)
__device__ __forceinline__ void rcx_flag(u32* status, u32 what, u64 blk)
{
    atomicOr(&status[0], what);
    atomicMin(&status[1], blk > 0xFFFFFFFEull ? 0xFFFFFFFEu : (u32)blk);
}

__device__ __forceinline__ u32 rcx_wave_max(u32 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        u32 other = (u32)__shfl_xor((int)v, o, 64);
        v = v > other ? v : other;
    }
    return v;
}

__device__ __forceinline__ u32 rcx_byte_of(const U4& w, u32 j)
{
    const u32 word = (j < 4) ? w.x : (j < 8) ? w.y : (j < 12) ? w.z : w.w;
    return (word >> (8 * (j & 3))) & 0xFFu;
}

// ===========================================================================
// Size prefix: offsets[b] = sum_{i<b} sizes[i], offsets[nblocks] = total.
// One workgroup of 1024 threads; wave scans via DPP shuffles, 16 wave totals via LDS.
// ===========================================================================
template <class G = RcxBlocks>
__global__ __launch_bounds__(1024) void rcx_scan_sizes_k(const u32* __restrict__ sizes, u64 nblocks, u64* __restrict__ offsets,
                                                         u64 dst_cap, u32* status, const G g = G())
{
    __shared__ u64 wave_total[16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 per = (nblocks + 1023) / 1024;
    const u64 first = (u64)tid * per;
    const u64 last = (first + per) < nblocks ? (first + per) : nblocks;
    u64 mine = 0;
    for (u64 b = first; b < last; ++b) mine += rcx_size_of(g, sizes, b);
    // inclusive wave scan
    u64 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u64 up = (u64)__shfl_up((unsigned long long)incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    u64 before = 0;
    for (u32 w = 0; w < wave; ++w) before += wave_total[w];
    u64 run = before + incl - mine;
    for (u64 b = first; b < last; ++b) {
        offsets[b] = run;
        run += rcx_size_of(g, sizes, b);
    }
    if (tid == 1023) {
        offsets[nblocks] = before + incl;
        if (before + incl > dst_cap) rcx_flag(status, RCX_ST_CAPACITY, nblocks);
    }
}

// ===========================================================================
// Encode, pass 2: slot b -> dst + offsets[b].  One workgroup per block; the
// destination is written in aligned 16-byte pieces, the (4-byte aligned) source
// words are byte-shifted into place.
// ===========================================================================
template <class G = RcxBlocks>
__global__ __launch_bounds__(256) void rcx_scatter_k(const u8* __restrict__ slots, u64 slot, const u32* __restrict__ sizes,
                                                     const u64* __restrict__ offsets, u8* __restrict__ dst, u64 dst_cap,
                                                     const u32* __restrict__ starts, const G g = G())
{
    const u64 blk = blockIdx.x;
    if constexpr (G::planned) { // the launch is shaped for the most entries there can be: behind the laid-out ones, or a hole
        if (blk >= (u64)g.nlive[0] || g.len[blk] == 0) return;
        RCX_ENTRY_SLOTS(g, blk, slots, slot);
    }
    const u32 size = sizes[blk];
    const u64 off = offsets[rcx_id(g, blk)]; // (the table is in the caller's order, the slots in work order)
    if (off + size > dst_cap) return; // flagged by the scan
    // the stream begins at the start of its slot (range coders) or wherever the backward-writing rANS encoders got to
    const u8* s = slots + blk * slot + (starts ? starts[blk] : 0u);
    u8* d = dst + off;
    const u32 tid = threadIdx.x;
    u32 head = (u32)((0 - reinterpret_cast<uintptr_t>(d)) & 15u);
    if (head > size) head = size;
    if (tid < head) d[tid] = s[tid];
    const u32 nvec = (size - head) >> 4;
    const uintptr_t from = reinterpret_cast<uintptr_t>(s) + head;
    const u32 sh = (u32)(from & 3u);
    const u32* w0p = reinterpret_cast<const u32*>(from & ~(uintptr_t)3);
    for (u32 v = tid; v < nvec; v += 256) {
        const u32* w = w0p + 4 * v;
        const u32 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        U4 out;
        out.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
        out.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
        out.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
        out.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
        *reinterpret_cast<U4*>(d + head + 16u * v) = out;
    }
    const u32 done = head + (nvec << 4);
    if (tid < size - done) d[done + tid] = s[done + tid];
}

#include "rcx_adaptive.hpp"
#include "rcx_quad.hpp"
#include "rcx_mc.hpp"
#if defined(RCX_WITH_VARIANTS) // superseded kernels, kept for comparison: only in the diagnostic build (build.py build_variants)
#include "variants/rcx_variants.hpp"
#endif
#include "rcx_static.hpp"
#include "rcx_rans.hpp"
#include "rcx_bwt.hpp"
#include "rcx_crc.hpp"
#include "rcx_stats.hpp"
#include "rcx_planes.hpp"
#include "rcx_stored.hpp"
