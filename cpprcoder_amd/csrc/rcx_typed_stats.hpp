// rcx_typed_stats.hpp -- the order-0 cost of every candidate transform of every item, in one pass over source and base
// (include/rcx_typed_stats.h): none, delta, zigzag (rcx_predict.hpp), xor, sub, subzz against the base span (rcx_base.hpp).
//
//     cost[6 * id + c] = sum over the W planes p of the item under candidate c of  n_p * L(n_p) - sum of f * L(f)
// with n_p = m = len / W bytes, the last plane with the len % W tail bytes as well (the source's values), f the plane's 256
// counts and L = rcx_log2_q16 (rcx_stats.hpp): what rcx_stats_items_device gives for the sub-items behind
// rcx_base_items_split_device with that candidate, word for word, without writing the transform anywhere.
//
// One kernel, instantiated per width W, a WORKGROUP TO AN ITEM on a fixed grid that loops over the width's entries, longest
// first (the plan below).  A lane's unit is the 16 elements of rcx_base.hpp -- W 16-byte loads of the source at a byte
// address (rcx_load16_any) and, if an op is asked for, W of the base at the same index.  The element in front of a unit is
// the neighbouring lane's last one (one shuffle); lane 0 of a wave loads it, and it is 0 in front of the item.  Per asked
// candidate -- the mask is the item's, so the branch is scalar -- the residual unit is rcx_predict_unit's or rcx_base_unit's,
// rcx_planes_unit turns it into W planes of 16 bytes, and each plane goes into the table of (candidate, plane) in LDS.
// What is not a whole unit, the last m % 16 elements and the tail bytes, goes one element (one byte) a lane.
//
// LDS.  One table set per workgroup, shared by its waves: 6 * W tables of 256 words, 6 KiB at width 1 and 48 KiB at width 8.
// Per-wave copies as in rcx_stats_k would be 192 KiB at width 8, more than a compute unit has.  A workgroup is 256 threads at
// every width: the unit's registers (91 VGPRs at width 4, 144 at width 8) allow five and three waves a SIMD, which is five and
// three workgroups a compute unit on 120 and 144 KiB; 512 threads a set would hold fewer waves, not more.  Only asked
// candidates are counted, read out and cleared.
//
// Skew is the normal case: an item equal to its base is all zeros under all three ops, one near it has high planes of 0x00
// and 0xFF.  All 16 bytes a lane adds to a table are of one plane, so a run of equal neighbours is one add of its length
// (rcx_stats_add16's merge): a constant plane costs a lane one ds_add where uniform bytes cost sixteen.
//
// Readout: behind a barrier thread t takes entries t, t + T, .. of each asked candidate's W * 256 counts, clears them and
// sums f * L(f) (rcx_stats_term); a wave sum, one partial per wave and candidate through LDS, and threads 0 .. 5 store the
// item's six words, 0 for a candidate nobody asked for.  An item of length 0 stores six zeros.
//
// The kernel reads exactly the entries' bytes, the whole elements of the base spans of the entries with an op bit, and
// writes exactly six words per entry.  No floating point, no inline assembly, no scratch; all offsets are 64-bit.
#pragma once

#include <algorithm>
#include <vector>

#include "rcx_base.hpp"
#include "rcx_stats.hpp"
#include "rcx_typed_items.hpp"

#define RCX_TSTATS_CANDS 6u
#define RCX_TSTATS_PRED_BITS 0x06u // delta, zigzag
#define RCX_TSTATS_OP_BITS 0x38u   // xor, sub, subzz
#define RCX_TSTATS_THREADS 256u

// ---- the plan (host; plain C++) ---------------------------------------------------------------------------------------------
// Every item has an entry, the empty ones too (their six words are 0).  Entries are grouped by width and, within a width,
// longest first, equal lengths in the caller's order: the one long item of a skewed batch starts first.
struct RcxTypedStatsPlan {
    u64 nent = 0;
    u32 first[5] = {}; // entries of width 1 << k: first[k] .. first[k + 1]
    u64 o_at = 0, o_bat = 0, o_len = 0, o_id = 0, o_mask = 0, bytes = 0;
};

struct RcxTypedStatsTables {
    const u64* at;   // [nent] byte offset of the entry in the source
    const u64* bat;  // [nent] ... of its span in the base (0 where no op is asked for)
    const u32* len;  // [nent]
    const u32* id;   // [nent] the item in the caller's order
    const u8* mask;  // [nent]
};

inline void rcx_typed_stats_plan(const u64* offs, const u64* boffs, const u8* widths, const u8* masks, u64 nitems, std::vector<u64>& mem, RcxTypedStatsPlan& p)
{
    std::vector<u64> keys[4];
    for (u64 i = 0; i < nitems; ++i) {
        const u32 w = widths[i], k = w == 1 ? 0u : w == 2 ? 1u : w == 4 ? 2u : 3u;
        keys[k].push_back(((u64)(0xFFFFFFFFu - (u32)(offs[i + 1] - offs[i])) << 32) | i);
    }
    p = RcxTypedStatsPlan();
    p.nent = nitems;
    u64 o = 0;
    p.o_at = o, o += nitems * sizeof(u64);
    p.o_bat = o, o += nitems * sizeof(u64);
    p.o_len = o, o += nitems * sizeof(u32);
    p.o_id = o, o += nitems * sizeof(u32);
    p.o_mask = o, o += nitems;
    p.bytes = o;
    mem.resize((o + 7) / 8);
    u8* const h = reinterpret_cast<u8*>(mem.data());
    u64 *const at = reinterpret_cast<u64*>(h + p.o_at), *const bat = reinterpret_cast<u64*>(h + p.o_bat);
    u32 *const len = reinterpret_cast<u32*>(h + p.o_len), *const id = reinterpret_cast<u32*>(h + p.o_id);
    u8* const mask = h + p.o_mask;
    u64 e = 0;
    for (u32 k = 0; k < 4; ++k) {
        p.first[k] = (u32)e;
        rcx_typed_longest_first(keys[k]);
        for (const u64 key : keys[k]) {
            const u64 i = key & 0xFFFFFFFFull;
            at[e] = offs[i];
            len[e] = (u32)(offs[i + 1] - offs[i]);
            bat[e] = (masks[i] & RCX_TSTATS_OP_BITS) && len[e] ? boffs[i] : 0;
            id[e] = (u32)i;
            mask[e] = masks[i];
            ++e;
        }
    }
    p.first[4] = (u32)e;
}

inline RcxTypedStatsTables rcx_typed_stats_tables(const u8* base, const RcxTypedStatsPlan& p)
{
    RcxTypedStatsTables t;
    t.at = reinterpret_cast<const u64*>(base + p.o_at);
    t.bat = reinterpret_cast<const u64*>(base + p.o_bat);
    t.len = reinterpret_cast<const u32*>(base + p.o_len);
    t.id = reinterpret_cast<const u32*>(base + p.o_id);
    t.mask = base + p.o_mask;
    return t;
}

#if !defined(RCX_HOST_SIM)

// the 16 bytes of one plane into its table, every run of equal neighbours as one add (rcx_stats_add16 on four words)
__device__ __forceinline__ void rcx_typed_stats_add16(u32* tab, const u32* w)
{
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

// a residual unit, 4 * W words in memory order, into the W tables of its candidate
template <u32 W>
__device__ __forceinline__ void rcx_typed_stats_count_unit(u32 (*tab)[256], const u32 (&r)[4 * W])
{
    if constexpr (W == 1) {
        rcx_typed_stats_add16(tab[0], r);
    } else {
        u32 o[4 * W];
        rcx_planes_unit<W, false>(r, o);
#pragma unroll
        for (u32 p = 0; p < W; ++p) rcx_typed_stats_add16(tab[p], &o[4 * p]);
    }
}

// one residual element, its byte p into table p
template <u32 W>
__device__ __forceinline__ void rcx_typed_stats_count_elem(u32 (*tab)[256], u64 v)
{
#pragma unroll
    for (u32 p = 0; p < W; ++p) atomicAdd(&tab[p][(u32)(v >> (8u * p)) & 255u], 1u);
}

template <u32 W>
__device__ __forceinline__ u64 rcx_typed_stats_load_elem(const u8* p)
{
    if constexpr (W == 1) return *p;
    else return rcx_load_elem<W>(p);
}

// ===========================================================================
// The entries first .. first + count - 1 of the tables, all of width W: six cost words each.
// ===========================================================================
template <u32 W>
__global__ __launch_bounds__(RCX_TSTATS_THREADS) void rcx_typed_stats_k(const u8* __restrict__ src, const u8* __restrict__ ref, RcxTypedStatsTables t,
                                                                           u32 first, u32 count, u64* __restrict__ cost)
{
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "width 1, 2, 4 or 8");
    constexpr u32 T = RCX_TSTATS_THREADS, WAVES = T / 64u, C = RCX_TSTATS_CANDS;
    __shared__ u32 tab[C][W][256];
    __shared__ u64 part[WAVES][C];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u32* const flat = &tab[0][0][0];
    for (u32 i = tid; i < C * W * 256u; i += T) flat[i] = 0;
    __syncthreads();
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        // (the entry's fields are the same in every thread: the branches on them are scalar, the barriers met by all)
        const u32 e = first + k, len = t.len[e], mask = t.mask[e];
        const u64 at = t.at[e], bat = t.bat[e];
        const u32 m = len / W, r = len - m * W, units = m >> 4;
        const u8* const s = src + at;
        const u8* const b = ref + bat; // (not read unless an op is asked for)
        for (u32 u0 = wave * 64u; u0 < units; u0 += T) {
            const u32 u = u0 + lane;
            const bool have = u < units;
            u32 x[4 * W] = {}, y[4 * W] = {};
            if (have) {
#pragma unroll
                for (u32 i = 0; i < W; ++i) rcx_load16_any(s + (u64)u * (16u * W) + 16u * i, &x[4 * i]);
                if (mask & RCX_TSTATS_OP_BITS) {
#pragma unroll
                    for (u32 i = 0; i < W; ++i) rcx_load16_any(b + (u64)u * (16u * W) + 16u * i, &y[4 * i]);
                }
            }
            if (mask & 1u) {
                if (have) rcx_typed_stats_count_unit<W>(tab[0], x);
            }
            if constexpr (W > 1) {
                if (mask & RCX_TSTATS_PRED_BITS) {
                    typedef typename RcxElem<W>::T E;
                    E prev = (E)__shfl_up((unsigned long long)rcx_elem_get<W>(x, 15), 1, 64);
                    if (lane == 0) prev = u && have ? rcx_load_elem<W>(s + (u64)u * (16u * W) - W) : (E)0;
                    if (have) {
                        u32 d[4 * W];
                        if (mask & 2u) {
                            rcx_predict_unit<W, false>(x, prev, d);
                            rcx_typed_stats_count_unit<W>(tab[1], d);
                        }
                        if (mask & 4u) {
                            rcx_predict_unit<W, true>(x, prev, d);
                            rcx_typed_stats_count_unit<W>(tab[2], d);
                        }
                    }
                }
            }
            if (have) {
                u32 d[4 * W];
                if (mask & 8u) {
                    rcx_base_unit<W, 0, false>(x, y, d);
                    rcx_typed_stats_count_unit<W>(tab[3], d);
                }
                if (mask & 16u) {
                    rcx_base_unit<W, 1, false>(x, y, d);
                    rcx_typed_stats_count_unit<W>(tab[4], d);
                }
                if (mask & 32u) {
                    rcx_base_unit<W, 2, false>(x, y, d);
                    rcx_typed_stats_count_unit<W>(tab[5], d);
                }
            }
        }
        // behind the whole units: element 16 * units + tid, then tail byte tid - 16
        if (tid < (m & 15u)) {
            const u32 el = (units << 4) + tid;
            const u64 v = rcx_typed_stats_load_elem<W>(s + (u64)el * W);
            if (mask & 1u) rcx_typed_stats_count_elem<W>(tab[0], v);
            if constexpr (W > 1) {
                if (mask & RCX_TSTATS_PRED_BITS) {
                    typedef typename RcxElem<W>::T E;
                    const E before = el ? rcx_load_elem<W>(s + (u64)el * W - W) : (E)0;
                    const E d = (E)((E)v - before) & rcx_elem_mask<W>();
                    if (mask & 2u) rcx_typed_stats_count_elem<W>(tab[1], d);
                    if (mask & 4u) rcx_typed_stats_count_elem<W>(tab[2], rcx_zigzag<W>(d));
                }
            }
            if (mask & RCX_TSTATS_OP_BITS) {
                const u64 o = rcx_typed_stats_load_elem<W>(b + (u64)el * W);
                if (mask & 8u) rcx_typed_stats_count_elem<W>(tab[3], rcx_base_elem<W, 0, false>(v, o));
                if (mask & 16u) rcx_typed_stats_count_elem<W>(tab[4], rcx_base_elem<W, 1, false>(v, o));
                if (mask & 32u) rcx_typed_stats_count_elem<W>(tab[5], rcx_base_elem<W, 2, false>(v, o));
            }
        } else if (tid >= 16u && tid - 16u < r) {
            const u32 c = s[(u64)m * W + (tid - 16u)];
#pragma unroll
            for (u32 q = 0; q < C; ++q)
                if (mask >> q & 1u) atomicAdd(&tab[q][W - 1][c], 1u);
        }
        __syncthreads();
#pragma unroll
        for (u32 q = 0; q < C; ++q) {
            if (!(mask >> q & 1u)) continue;
            u32* const mine = &tab[q][0][0];
            u64 sum = 0;
#pragma unroll
            for (u32 i = tid; i < W * 256u; i += T) {
                const u32 f = mine[i];
                mine[i] = 0;
                sum += rcx_stats_term(f);
            }
            sum = rcx_stats_wave_sum(sum);
            if (lane == 0) part[wave][q] = sum;
        }
        __syncthreads();
        if (tid < C) {
            u64 v = 0;
            if (mask >> tid & 1u) {
                v = (u64)(W - 1u) * rcx_stats_term(m) + rcx_stats_term(m + r);
#pragma unroll
                for (u32 w = 0; w < WAVES; ++w) v -= part[w][tid];
            }
            cost[(u64)t.id[e] * C + tid] = v;
        }
        __syncthreads(); // (part and the tables are the next entry's)
    }
}

#endif // !RCX_HOST_SIM
