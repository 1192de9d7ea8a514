// rcx_stats.hpp -- order-0 statistics of every work entry (block or item) on the GPU (include/rcx_stats.h): the 256 byte
// counts and, from them, the entry's order-0 cost in bits times 65536.
//
//     hist[id * 256 + c] = how many bytes of the entry equal c
//     cost[id]           = m * L(m) - sum over f_c > 0 of f_c * L(f_c),   m = the entry's length, f_c its counts
// L(x) = floor(log2(x) * 65536) by sixteen square-and-compare steps (rcx_log2_q16 below: the header's recurrence, word for
// word), so every figure is an integer and the same on every machine.
//
// One kernel for both geometries, on a fixed grid that loops over WORK UNITS:
//     a LONG entry (more than RCX_STATS_SHORT bytes) is a unit of its own, counted by the whole workgroup: thread t takes
//         the 16 bytes at 16 * (t + 256 * row), RCX_STATS_ROWS rows in flight, and adds each byte to its WAVE's table in
//         LDS (four tables of 256 words, ds_add_u32: no wave waits for another one's atomics).  Behind a barrier thread c
//         adds the four counts of symbol c, clears them for the next unit, stores the row of hist and takes f * L(f); a
//         wave reduction, four partial sums through LDS and one 64-bit store finish the entry.
//     SHORT entries go four to a unit, one to a wave, as the CRC kernel packs them (rcx_crc.hpp): the wave counts into its
//         own table, lane l finishes symbols l, l + 64, l + 128 and l + 192, and lane 0 stores the cost.
// The host says where the short ones begin: with blocks all entries are of one kind; with items the work order is longest
// first (rcx_crc_api.hpp, plan_crc_items), so the long ones are the first `nlong` entries.  (In the caller's order --
// RCX_ITEMS_ORDER=0, diagnostic -- every entry is taken as long as soon as one is: that path counts any length.)
//
// Every 16-byte load goes to a byte address (RcxU4AnyAlign, rcx_geom.hpp); the up to 15 bytes behind the last whole 16 are
// read one by one.  The kernel reads exactly the entries' bytes and writes exactly the two tables, either of which may be
// absent.  An entry of length 0 has a row of zeros and cost 0.
//
// Skew.  A plane of one repeated byte sends all 64 lanes of every ds_add to one address, which the LDS serialises; the
// predictor makes such planes (measured: 3.48 ms a GiB against 0.30 ms for uniform bytes).  So a lane adds each run of equal
// neighbours among its 16 bytes at once: one add of 16 instead of sixteen of 1 on such a plane (0.36 ms), the same
// sixteen adds on bytes that do not repeat (0.31 ms).  DESIGN.md section 13 has the table.
// No floating point, no inline assembly, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_geom.hpp"

#define RCX_STATS_WAVES 4
#define RCX_STATS_THREADS (64 * RCX_STATS_WAVES)
#define RCX_STATS_ROWS 4      // 16-byte loads a thread has in flight
#define RCX_STATS_SHORT 1024u // an entry of at most this many bytes is one wave's: a single row of 16-byte loads

// floor(log2(x) * 65536) for 1 <= x < 2^32 (the contract asks for x <= 2^24): include/rcx_stats.h has this as C
RCX_HD u32 rcx_log2_q16(u32 x)
{
    const u32 e = 31u - (u32)__builtin_clz(x);
    u64 m = (u64)x << (31u - e); // 2^31 <= m < 2^32: x / 2^e in Q31
    u32 r = e;
    for (int i = 0; i < 16; ++i) {
        m = (m * m) >> 31;       // the square, in [2^31, 2^33)
        const u32 bit = (u32)(m >> 32);
        m >>= bit;
        r = 2u * r + bit;
    }
    return r;
}

// f * L(f), 0 for a symbol that does not occur (and for an empty entry)
RCX_HD u64 rcx_stats_term(u32 f) { return f ? (u64)f * rcx_log2_q16(f) : 0ull; }

__device__ __forceinline__ u64 rcx_stats_wave_sum(u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// the 16 bytes of v into the table, every run of equal neighbours as one add
__device__ __forceinline__ void rcx_stats_add16(u32* tab, const RcxU4AnyAlign& v)
{
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u32 run = 1;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        const u32 c = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
        const u32 next = j < 15 ? (w[(j + 1) >> 2] >> (8u * ((j + 1) & 3u))) & 255u : 256u;
        if (c == next) {
            ++run;
        } else {
            atomicAdd(&tab[c], run);
            run = 1;
        }
    }
}

// The bytes [p, p + len) into `tab` by `threads` threads of which this is thread t: whole 16-byte pieces, then the rest.
__device__ __forceinline__ void rcx_stats_count(u32* tab, const u8* p, u32 len, u32 t, u32 threads)
{
    const u32 nvec = len >> 4;
    const RcxU4AnyAlign* q = reinterpret_cast<const RcxU4AnyAlign*>(p);
    u32 v = t;
    for (; v + (RCX_STATS_ROWS - 1) * threads < nvec; v += RCX_STATS_ROWS * threads) {
        RcxU4AnyAlign x[RCX_STATS_ROWS];
#pragma unroll
        for (u32 j = 0; j < RCX_STATS_ROWS; ++j) x[j] = q[v + j * threads];
#pragma unroll
        for (u32 j = 0; j < RCX_STATS_ROWS; ++j) rcx_stats_add16(tab, x[j]);
    }
    for (; v < nvec; v += threads) rcx_stats_add16(tab, q[v]);
    const u32 i = (nvec << 4) + t;
    if (i < len) atomicAdd(&tab[p[i]], 1u);
}

// ===========================================================================
// Counts and cost of every work entry.  Units 0 .. nlong - 1 are the long entries of the same index, a workgroup to each;
// unit nlong + k is the short entries nlong + 4k .. nlong + 4k + 3, a wave to each.  id = the block, or the item.
// ===========================================================================
template <class G = RcxBlocks>
__global__ __launch_bounds__(RCX_STATS_THREADS) void rcx_stats_k(const u8* __restrict__ src, u64 n, u32 block, u64 nblocks, u64 nlong,
                                                                 u32* __restrict__ hist, u64* __restrict__ cost, const G g = G())
{
    __shared__ u32 tab[RCX_STATS_WAVES][256];
    __shared__ u64 part[RCX_STATS_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (u32 w = 0; w < RCX_STATS_WAVES; ++w) tab[w][tid] = 0;
    __syncthreads();
    const u64 units = nlong + (nblocks - nlong + RCX_STATS_WAVES - 1) / RCX_STATS_WAVES;
    for (u64 unit = blockIdx.x; unit < units; unit += gridDim.x) {
        if (unit < nlong) { // (the same for every thread of the workgroup: the barriers below are met by all)
            const u64 blk = unit;
            RCX_ENTRY(g, blk, nblocks, n, block);
            (void)live;
            rcx_stats_count(tab[wave], src + at, len, tid, RCX_STATS_THREADS);
            __syncthreads();
            u32 f = 0;
#pragma unroll
            for (u32 w = 0; w < RCX_STATS_WAVES; ++w) {
                f += tab[w][tid];
                tab[w][tid] = 0;
            }
            const u64 id = rcx_id(g, blk);
            if (hist) hist[id * 256u + tid] = f;
            const u64 sum = rcx_stats_wave_sum(rcx_stats_term(f));
            if (lane == 0) part[wave] = sum;
            __syncthreads();
            if (tid == 0 && cost) cost[id] = rcx_stats_term(len) - (part[0] + part[1] + part[2] + part[3]);
        } else {
            const u64 blk = nlong + (unit - nlong) * RCX_STATS_WAVES + wave;
            RCX_ENTRY(g, blk, nblocks, n, block);
            if (live) rcx_stats_count(tab[wave], src + at, len, lane, 64u);
            __syncthreads(); // (a wave's own atomics would be in order without it; the table is clean for a long unit behind this one)
            if (live) {
                const u64 id = rcx_id(g, blk);
                u64 sum = 0;
#pragma unroll
                for (u32 k = 0; k < 4; ++k) {
                    const u32 c = lane + 64u * k, f = tab[wave][c];
                    tab[wave][c] = 0;
                    if (hist) hist[id * 256u + c] = f;
                    sum += rcx_stats_term(f);
                }
                sum = rcx_stats_wave_sum(sum);
                if (lane == 0 && cost) cost[id] = rcx_stats_term(len) - sum;
            }
            __syncthreads();
        }
    }
}
