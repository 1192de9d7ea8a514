// rcx_planes.hpp -- the byte-plane filter for typed data (include/rcx_planes.h): the bytes of W-byte elements, taken
// apart into W planes in front of an order-0 coder (split) and put together again behind the decoder (join); and the
// forward half of the delta predictor (include/rcx_predict.h), which is the same kernel with a difference in front of the
// transpose.  Here: the unit transposes, the element arithmetic both directions of the predictor share, and the one
// kernel rcx_planes_k<W, JOIN, PRED>.  rcx_predict.hpp has what only the predictor's inverse uses.
//
// A SUPERBLOCK is W * B source bytes, B elements, where B is the block size the coder will use.  Superblock s begins at
// at = s * W * B and has R = min(W * B, n - at) bytes, m = R / W whole elements:
//     plane p (0 <= p < W) = src[at + p + k * W], k = 0 .. m - 1   ->   dst[at + p * m + k]
//     the R % W bytes behind the last whole element keep their places, dst[at + m * W ..  at + R)
// In a whole superblock m = B: coder block s * W + p of the output is exactly plane p.  Join is the inverse.
//
// The kernel: a lane's UNIT is 16 elements.  For split it issues W 16-byte loads of 16 * W consecutive source bytes,
// transposes the 16 x W bytes in registers with v_perm_b32 (rcx_perm: 8, 32 and 64 of them for W = 2, 4, 8) and issues
// W 16-byte stores, one per plane; join mirrors that.  Consecutive lanes take consecutive units, so a wave's loads are
// W KiB contiguous and its stores 1 KiB contiguous per plane (as long as they stay inside one superblock).  A fixed
// grid loops over the units of all superblocks; a workgroup takes RCX_PLANES_U4 / W rows of 256 units at a time and has
// all their loads in flight before the first transpose.  What is not a whole unit -- the last m % 16 elements of a
// superblock and its R % W tail bytes -- goes byte by byte behind the unit loop, one byte a lane.
//
// PRED = 1 (delta) or 2 (delta, then zigzag), split only: every element becomes its difference to the element in front,
// modulo 2^(8W), restarting in every superblock.  The difference is taken in registers between load and transpose; the
// element in front of a unit comes from one more W-byte load at (the unit's first element - W), a line the neighbouring
// lane fetches anyway, and is 0 for the first unit of a superblock.  A rest byte's lane loads its element and the one in
// front.  PRED = 0 compiles to the filter alone; the inverse with a predictor is a scan, rcx_predict_join_k.
//
// Alignment: every 16-byte access goes to a byte address (RcxU4AnyAlign, rcx_geom.hpp: global_load / global_store_dwordx4
// on a 1-aligned type, which gfx950 serves).  When source, destination and B are multiples of 16 every one of them is
// aligned and costs what an aligned access costs; there is one code path, not two.
// The kernel reads exactly [src, src + n) and writes exactly [dst, dst + n).  No LDS, no floating point, no inline assembly.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "rcx_lane.hpp"

#define RCX_PLANES_THREADS 256
#define RCX_PLANES_U4 16 // 16-byte registers a lane has in flight: 8, 4, 2 units for W = 2, 4, 8

// 4 x 4 bytes transposed: out word i byte j = in word j byte i.  Eight v_perm_b32; its own inverse.
RCX_DEV void rcx_transpose4(u32 a, u32 b, u32 c, u32 d, u32& o0, u32& o1, u32& o2, u32& o3)
{
    const u32 ab_lo = rcx_perm(b, a, 0x05010400u); // a0 b0 a1 b1
    const u32 ab_hi = rcx_perm(b, a, 0x07030602u); // a2 b2 a3 b3
    const u32 cd_lo = rcx_perm(d, c, 0x05010400u);
    const u32 cd_hi = rcx_perm(d, c, 0x07030602u);
    o0 = rcx_perm(cd_lo, ab_lo, 0x05040100u); // a0 b0 c0 d0
    o1 = rcx_perm(cd_lo, ab_lo, 0x07060302u); // a1 b1 c1 d1
    o2 = rcx_perm(cd_hi, ab_hi, 0x05040100u);
    o3 = rcx_perm(cd_hi, ab_hi, 0x07060302u);
}

// One unit in registers: w[0 .. 4W) are the unit's 16 * W bytes as little-endian words, in memory order.
// Split: in = 16 elements, out = W planes of 16 bytes (plane p = o[4p .. 4p + 4)).  Join: the other way.
template <u32 W, bool JOIN>
RCX_DEV void rcx_planes_unit(const u32 (&w)[4 * W], u32 (&o)[4 * W])
{
    if constexpr (W == 2) {
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
            if (JOIN) { // planes a = w[q], b = w[4 + q]: elements 4q .. 4q + 3
                o[2 * q] = rcx_perm(w[4 + q], w[q], 0x05010400u);     // a0 b0 a1 b1
                o[2 * q + 1] = rcx_perm(w[4 + q], w[q], 0x07030602u); // a2 b2 a3 b3
            } else { // words 2q, 2q + 1 = elements 4q .. 4q + 3
                o[q] = rcx_perm(w[2 * q + 1], w[2 * q], 0x06040200u);     // the even bytes
                o[4 + q] = rcx_perm(w[2 * q + 1], w[2 * q], 0x07050301u); // the odd bytes
            }
        }
    } else if constexpr (W == 4) {
#pragma unroll
        for (u32 q = 0; q < 4; ++q) { // elements 4q .. 4q + 3 are words 4q .. 4q + 3; their byte p is word q of plane p
            if (JOIN) rcx_transpose4(w[q], w[4 + q], w[8 + q], w[12 + q], o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
            else rcx_transpose4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], o[q], o[4 + q], o[8 + q], o[12 + q]);
        }
    } else { // W == 8: element e is words 2e (bytes 0 .. 3, planes 0 .. 3) and 2e + 1 (planes 4 .. 7)
        static_assert(W == 8, "width 2, 4 or 8");
#pragma unroll
        for (u32 h = 0; h < 2; ++h) {
#pragma unroll
            for (u32 q = 0; q < 4; ++q) {
                if (JOIN)
                    rcx_transpose4(w[16 * h + q], w[16 * h + 4 + q], w[16 * h + 8 + q], w[16 * h + 12 + q], o[8 * q + h], o[8 * q + 2 + h],
                                   o[8 * q + 4 + h], o[8 * q + 6 + h]);
                else
                    rcx_transpose4(w[8 * q + h], w[8 * q + 2 + h], w[8 * q + 4 + h], w[8 * q + 6 + h], o[16 * h + q], o[16 * h + 4 + q],
                                   o[16 * h + 8 + q], o[16 * h + 12 + q]);
            }
        }
    }
}

// ---- the predictor's arithmetic of one unit, forward: plain functions, also compiled for the host (tests/sim/predict_sim.cpp)
// An element of W bytes lives in the low 8W bits of a T: u32 for W = 2 and 4, u64 for W = 8.
template <u32 W>
struct RcxElem {
    typedef u32 T;
};
template <>
struct RcxElem<8> {
    typedef u64 T;
};

template <u32 W>
RCX_DEV typename RcxElem<W>::T rcx_elem_mask()
{
    typedef typename RcxElem<W>::T T;
    return W == 2 ? (T)0xFFFFu : (T) ~(T)0;
}

// z = (d << 1) XOR (0 - (d >> (8W - 1))), logical shifts; d < 2^(8W)
template <u32 W>
RCX_DEV typename RcxElem<W>::T rcx_zigzag(typename RcxElem<W>::T d)
{
    typedef typename RcxElem<W>::T T;
    return ((T)(d << 1) ^ (T)((T)0 - (T)(d >> (8 * W - 1)))) & rcx_elem_mask<W>();
}

// Element k (0 .. 15) of a unit held as 4W little-endian words in memory order, and the other way.
template <u32 W>
RCX_DEV typename RcxElem<W>::T rcx_elem_get(const u32 (&w)[4 * W], u32 k)
{
    typedef typename RcxElem<W>::T T;
    if constexpr (W == 2) return (w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
    else if constexpr (W == 4) return w[k];
    else return (T)w[2 * k] | ((T)w[2 * k + 1] << 32);
}

template <u32 W>
RCX_DEV void rcx_elems_put(const typename RcxElem<W>::T (&e)[16], u32 (&w)[4 * W])
{
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        if constexpr (W == 2) {
            if (k & 1u) w[k >> 1] = (u32)e[k - 1] | ((u32)e[k] << 16);
        } else if constexpr (W == 4) {
            w[k] = e[k];
        } else {
            w[2 * k] = (u32)e[k];
            w[2 * k + 1] = (u32)(e[k] >> 32);
        }
    }
}

// Forward: out element k = in element k - in element k - 1 (`prev` in front of element 0), zigzagged if ZIGZAG.
template <u32 W, bool ZIGZAG>
RCX_DEV void rcx_predict_unit(const u32 (&in)[4 * W], typename RcxElem<W>::T prev, u32 (&out)[4 * W])
{
    typedef typename RcxElem<W>::T T;
    T d[16];
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        const T e = rcx_elem_get<W>(in, k);
        const T x = (T)(e - prev) & rcx_elem_mask<W>();
        d[k] = ZIGZAG ? rcx_zigzag<W>(x) : x;
        prev = e;
    }
    rcx_elems_put<W>(d, out);
}

#if !defined(RCX_HOST_SIM)
#include "rcx_geom.hpp"

__device__ __forceinline__ void rcx_load16_any(const u8* p, u32* w)
{
    const RcxU4AnyAlign v = *reinterpret_cast<const RcxU4AnyAlign*>(p);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
}

// W bytes at any byte address as an element (rcx_predict.hpp has the store).
template <class V>
struct __attribute__((packed, aligned(1))) RcxAnyAlign {
    V v;
};

template <u32 W>
__device__ __forceinline__ typename RcxElem<W>::T rcx_load_elem(const u8* p)
{
    if constexpr (W == 2) return reinterpret_cast<const RcxAnyAlign<uint16_t>*>(p)->v;
    else if constexpr (W == 4) return reinterpret_cast<const RcxAnyAlign<u32>*>(p)->v;
    else return reinterpret_cast<const RcxAnyAlign<u64>*>(p)->v;
}

// One step of a workgroup: units base + j * 256 + tid, j = 0 .. K - 1, all loads first.  GUARD = false: every one of
// them exists (no branch between the loads and the stores, so the waits count down load by load); GUARD = true: the
// last step of the call, where some do not.
template <u32 W, bool JOIN, u32 PRED, bool GUARD>
__device__ __forceinline__ void rcx_planes_step(const u8* __restrict__ src, u8* __restrict__ dst, u64 base, u64 total, u32 units, u64 nfull, u32 block,
                                                u32 m_last, u32 tid)
{
    constexpr u32 K = RCX_PLANES_U4 / W;
    // unit g lies in superblock g / units (the last one has no more units than a whole one), and is its unit g % units
    const u64 s0 = base / units;
    const u32 u0 = (u32)(base - s0 * units);
    u32 w[K][4 * W];
    [[maybe_unused]] typename RcxElem<W>::T prev[K];
    u64 to[K];
    u32 m[K];
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u32 off = u0 + j * RCX_PLANES_THREADS + tid; // < 2^20 + 2048
        const u32 ds = off / units;
        const u64 s = s0 + ds;
        const u32 u = off - ds * units;
        m[j] = s < nfull ? block : m_last;
        const u64 at = s * ((u64)W * block);
        const u64 elements = at + (u64)u * (16u * W), planes = at + 16ull * u; // plane p: + p * m
        to[j] = JOIN ? elements : planes;
        if constexpr (PRED != 0) prev[j] = 0; // the predictor restarts with the superblock
        if (!GUARD || base + j * RCX_PLANES_THREADS + tid < total) {
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(src + (JOIN ? planes + (u64)i * m[j] : elements + 16ull * i), &w[j][4 * i]);
            if constexpr (PRED != 0) {
                if (u) prev[j] = rcx_load_elem<W>(src + elements - W);
            }
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || base + j * RCX_PLANES_THREADS + tid < total) {
            u32 o[4 * W];
            if constexpr (PRED != 0) {
                u32 d[4 * W];
                rcx_predict_unit<W, PRED == 2>(w[j], prev[j], d);
                rcx_planes_unit<W, JOIN>(d, o);
            } else {
                rcx_planes_unit<W, JOIN>(w[j], o);
            }
#pragma unroll
            for (u32 i = 0; i < W; ++i)
                rcx_store16<true>(dst + to[j] + (JOIN ? 16ull * i : (u64)i * m[j]), U4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]});
        }
    }
}

// ===========================================================================
// nfull = n / (W * block), the whole superblocks (the host has it; everything else follows from it with 32-bit
// divisions and one 64-bit division per step, of a number that is the same for the whole workgroup).
// ===========================================================================
template <u32 W, bool JOIN, u32 PRED>
__global__ __launch_bounds__(RCX_PLANES_THREADS) void rcx_planes_k(const u8* __restrict__ src, u8* __restrict__ dst, u64 n, u32 block, u64 nfull)
{
    static_assert(PRED <= 2 && !(JOIN && PRED), "the inverse with a predictor is rcx_predict_join_k");
    constexpr u32 STEP = RCX_PLANES_U4 / W * RCX_PLANES_THREADS; // units a workgroup takes at a time
    const u64 super = (u64)W * block;                            // bytes of a whole superblock
    const u32 r_last = (u32)(n - nfull * super);                 // bytes of the ragged last one, < W * block <= 2^27
    const u32 m_last = r_last / W;
    const u32 units = block >> 4, units_last = m_last >> 4;      // whole units of a whole superblock (>= 1), of the last one
    const u64 total = nfull * units + units_last;
    const u32 tid = threadIdx.x;

    for (u64 base = (u64)blockIdx.x * STEP; base < total; base += (u64)gridDim.x * STEP) {
        if (base + STEP <= total) rcx_planes_step<W, JOIN, PRED, false>(src, dst, base, total, units, nfull, block, m_last, tid);
        else rcx_planes_step<W, JOIN, PRED, true>(src, dst, base, total, units, nfull, block, m_last, tid);
    }

    // What is left of every superblock behind its whole units, one byte a lane: (m % 16) elements (with a predictor each
    // against the element in front of it), then R % W tail bytes as they are.
    const u32 rest = (block & 15u) * W;                          // of a whole superblock (0 for blocks that are multiples of 16)
    const u32 rest_last = r_last - units_last * (16u * W);       // of the last one, < 17 * W
    const u64 rest_whole = nfull * rest, rest_total = rest_whole + rest_last;
    for (u64 t = (u64)blockIdx.x * RCX_PLANES_THREADS + tid; t < rest_total; t += (u64)gridDim.x * RCX_PLANES_THREADS) {
        u64 s = nfull;
        u32 j = (u32)(t - rest_whole), mm = m_last;
        if (t < rest_whole) {
            s = t / rest;
            j = (u32)(t - s * rest);
            mm = block;
        }
        const u64 at = s * super;
        const u32 e0 = mm & ~15u, in_elements = (mm - e0) * W;
        if (j < in_elements) {
            const u32 e = e0 + j / W, p = j % W;
            if constexpr (PRED != 0) {
                typedef typename RcxElem<W>::T T;
                const u8* element = src + at + (u64)e * W;
                const T here = rcx_load_elem<W>(element), front = e ? rcx_load_elem<W>(element - W) : (T)0;
                const T d = (T)(here - front) & rcx_elem_mask<W>();
                dst[at + (u64)p * mm + e] = (u8)((PRED == 2 ? rcx_zigzag<W>(d) : d) >> (8u * p));
            } else {
                const u64 element = at + (u64)e * W + p, plane = at + (u64)p * mm + e;
                dst[JOIN ? element : plane] = src[JOIN ? plane : element];
            }
        } else {
            const u64 i = at + (u64)mm * W + (j - in_elements);
            dst[i] = src[i];
        }
    }
}

#endif // !RCX_HOST_SIM
