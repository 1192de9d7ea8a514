// rcx_base.hpp -- residuals against a base buffer (include/rcx_base.h), fused with the byte-plane filter of rcx_planes.hpp:
// split = every element's residual against the base's element at the same place (xor, difference, or zigzagged
// difference), then the planes; join = the planes put together, then the inverse with the same base.  Superblocks, units
// and the plane layout are those of rcx_planes.hpp, whose unit transpose (rcx_planes_unit), byte-addressed 16-byte accesses
// (rcx_load16_any, rcx_store16<true>) and element loads this file reuses; the zigzag pair is that of rcx_planes.hpp /
// rcx_predict.hpp.  All arithmetic is modulo 2^(8W).  The stage is elementwise: no chain, no scan, both directions are the
// one kernel rcx_base_k<W, JOIN, OP>.
//
// The kernel: a lane's UNIT is 16 elements, 16 * W bytes.  Split issues W 16-byte loads of the source and W of the base at
// the same offsets, takes the residual in registers, transposes and issues W 16-byte stores, one per plane.  Join issues
// the W plane loads and the W base loads together, transposes, applies the inverse and stores 16 * W consecutive bytes.
// A workgroup takes RCX_BASE_ROWS(W) = RCX_BASE_U4 / (2 * W) rows of 256 units at a time and has all their loads -- source and base -- in
// flight before the first arithmetic: the base doubles what a row holds, so there are half as many rows as in
// rcx_planes_step and the same 16 16-byte registers a lane.  Width 1 has no planes and no superblocks: the buffer is one
// run of 16-byte units, eight rows a step.  What is not a whole unit -- the last m % 16 elements of a superblock and its
// R % W tail bytes, which keep the source's values -- goes one byte a lane behind the unit loop.
//
// THE OP IS WORD ARITHMETIC on the unit's 4 * W words as they were loaded, not element extraction:
//     xor    the raw words, every width
//     W = 4  one 32-bit subtract (add) a word; W = 8 subtract with borrow over a word pair
//     W = 2  the word as two 16-bit lanes of a vector type: packed 16-bit subtract, shift and xor
//     W = 1  four bytes a word without a borrow between them: with H = 0x80808080,
//            x - b = ((x | H) - (b & ~H)) ^ ((x ^ ~b) & H)      x + b = ((x & ~H) + (b & ~H)) ^ ((x ^ b) & H)
//            z(d) = ((d & ~H) << 1) ^ rcx_byte_fill(d & H)      z^-1(z) = ((z >> 1) & ~H) ^ rcx_byte_fill((z << 7) & H)
//            rcx_byte_fill(s) = s | (s - (s >> 7)): 0xFF in every byte whose top bit is set in s, without a multiply
//
// The kernel reads exactly [src, src + n) and [ref, ref + n) and writes exactly [dst, dst + n), at any alignment.  The grid
// is fixed and loops; all offsets are 64-bit.  No LDS, no floating point, no inline assembly, no wave waits for another.
#pragma once

#include "rcx_predict.hpp"

#define RCX_BASE_THREADS 256
#define RCX_BASE_U4 16 // 16-byte registers a lane has in flight, source and base together: 8, 4, 2, 1 rows for W = 1, 2, 4, 8
// Width 8 has one row in flight.  Two (-DRCX_BASE_ROWS8=2: 150 VGPRs, 3 waves a SIMD where one row has 7 and 6) were measured
// and are slower, split 0.70 - 0.74 ms a GiB against 0.65 - 0.67 (profiles/r15_base_rows8.jsonl).
#ifndef RCX_BASE_ROWS8
#define RCX_BASE_ROWS8 1
#endif
#define RCX_BASE_ROWS(W) ((W) == 8 ? RCX_BASE_ROWS8 : RCX_BASE_U4 / (2 * (W)))

// ---- the arithmetic of one unit: plain functions, also compiled for the host (tests/sim/base_sim.cpp) ------------------------
typedef uint16_t RcxU16x2 __attribute__((vector_size(4))); // a word as two 16-bit lanes

RCX_DEV RcxU16x2 rcx_as_u16x2(u32 x)
{
    RcxU16x2 v;
    __builtin_memcpy(&v, &x, 4);
    return v;
}

RCX_DEV u32 rcx_from_u16x2(RcxU16x2 v)
{
    u32 x;
    __builtin_memcpy(&x, &v, 4);
    return x;
}

// s has nothing but top bits of bytes: every byte with one becomes 0xFF (0x80 - 1 = 0x7F stays inside the byte).
RCX_DEV u32 rcx_byte_fill(u32 s) { return s | (s - (s >> 7)); }

// One word of W-byte elements (W = 1, 2, 4) against the base's word.  Forward: the residual; JOIN: the element back.
template <u32 W, u32 OP, bool JOIN>
RCX_DEV u32 rcx_base_word(u32 x, u32 b)
{
    static_assert(W == 1 || W == 2 || W == 4, "width 8 goes by word pairs");
    static_assert(OP == 1 || OP == 2, "xor is the raw words");
    if constexpr (W == 4) {
        if (JOIN) return (OP == 2 ? rcx_unzigzag<4>(x) : x) + b;
        return OP == 2 ? rcx_zigzag<4>(x - b) : x - b;
    } else if constexpr (W == 2) {
        const RcxU16x2 v = rcx_as_u16x2(x), r = rcx_as_u16x2(b);
        const RcxU16x2 zero = {0, 0}, one = {1, 1};
        if (JOIN) return rcx_from_u16x2((OP == 2 ? (RcxU16x2)((v >> 1) ^ (zero - (v & one))) : v) + r);
        const RcxU16x2 d = v - r;
        return rcx_from_u16x2(OP == 2 ? (RcxU16x2)((d << 1) ^ (zero - (d >> 15))) : d);
    } else {
        constexpr u32 H = 0x80808080u;
        if (JOIN) {
            const u32 d = OP == 2 ? ((x >> 1) & ~H) ^ rcx_byte_fill((x << 7) & H) : x;
            return ((d & ~H) + (b & ~H)) ^ ((d ^ b) & H);
        }
        const u32 d = ((x | H) - (b & ~H)) ^ ((x ^ ~b) & H);
        return OP == 2 ? ((d & ~H) << 1) ^ rcx_byte_fill(d & H) : d;
    }
}

// A unit held as 4 * W little-endian words in memory order, and the base's unit: forward, o = the residuals; JOIN, x holds
// residuals and o = the elements.
template <u32 W, u32 OP, bool JOIN>
RCX_DEV void rcx_base_unit(const u32 (&x)[4 * W], const u32 (&b)[4 * W], u32 (&o)[4 * W])
{
    static_assert(OP <= 2, "xor, sub or subzz");
    if constexpr (OP == 0) {
#pragma unroll
        for (u32 i = 0; i < 4 * W; ++i) o[i] = x[i] ^ b[i];
    } else if constexpr (W == 8) {
#pragma unroll
        for (u32 k = 0; k < 16; ++k) {
            const u64 e = (u64)x[2 * k] | ((u64)x[2 * k + 1] << 32), r = (u64)b[2 * k] | ((u64)b[2 * k + 1] << 32);
            const u64 v = JOIN ? (OP == 2 ? rcx_unzigzag<8>(e) : e) + r : (OP == 2 ? rcx_zigzag<8>(e - r) : e - r);
            o[2 * k] = (u32)v;
            o[2 * k + 1] = (u32)(v >> 32);
        }
    } else {
#pragma unroll
        for (u32 i = 0; i < 4 * W; ++i) o[i] = rcx_base_word<W, OP, JOIN>(x[i], b[i]);
    }
}

// One element in the low 8W bits, the scalar statement of the same: what the lanes behind the unit loop use.
template <u32 W, u32 OP, bool JOIN>
RCX_DEV u64 rcx_base_elem(u64 x, u64 b)
{
    constexpr u64 mask = ~0ull >> (64u - 8u * W);
    if (OP == 0) return x ^ b;
    if (JOIN) {
        const u64 d = OP == 2 ? ((x >> 1) ^ (0ull - (x & 1u))) & mask : x;
        return (d + b) & mask;
    }
    const u64 d = (x - b) & mask;
    return OP == 2 ? ((d << 1) ^ (0ull - (d >> (8u * W - 1u)))) & mask : d;
}

#if !defined(RCX_HOST_SIM)

// One step of a workgroup, W = 2, 4, 8: units first + j * 256 + tid, j = 0 .. K - 1, all loads of source and base first.
// GUARD = false: every one of them exists (no branch between the loads and the stores); GUARD = true: the last step.
template <u32 W, bool JOIN, u32 OP, bool GUARD>
__device__ __forceinline__ void rcx_base_step(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst, u64 first, u64 total, u32 units,
                                              u64 nfull, u32 block, u32 m_last, u32 tid)
{
    constexpr u32 K = RCX_BASE_ROWS(W);
    // unit g lies in superblock g / units (the last one has no more units than a whole one), and is its unit g % units
    const u64 s0 = first / units;
    const u32 u0 = (u32)(first - s0 * units);
    u32 w[K][4 * W], b[K][4 * W];
    u64 elements[K], planes[K];
    u32 m[K];
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u32 off = u0 + j * RCX_BASE_THREADS + tid; // < 2^20 + 1024
        const u32 ds = off / units;
        const u64 s = s0 + ds;
        const u32 u = off - ds * units;
        m[j] = s < nfull ? block : m_last;
        const u64 at = s * ((u64)W * block);
        elements[j] = at + (u64)u * (16u * W);
        planes[j] = at + 16ull * u; // plane p: + p * m
        if (!GUARD || first + j * RCX_BASE_THREADS + tid < total) {
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(src + (JOIN ? planes[j] + (u64)i * m[j] : elements[j] + 16ull * i), &w[j][4 * i]);
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(ref + elements[j] + 16ull * i, &b[j][4 * i]);
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || first + j * RCX_BASE_THREADS + tid < total) {
            u32 r[4 * W], o[4 * W];
            if (JOIN) {
                rcx_planes_unit<W, true>(w[j], r);
                rcx_base_unit<W, OP, true>(r, b[j], o);
            } else {
                rcx_base_unit<W, OP, false>(w[j], b[j], r);
                rcx_planes_unit<W, false>(r, o);
            }
#pragma unroll
            for (u32 i = 0; i < W; ++i)
                rcx_store16<true>(dst + (JOIN ? elements[j] + 16ull * i : planes[j] + (u64)i * m[j]), U4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]});
        }
    }
}

// The same for W = 1: unit g is bytes 16 g .. 16 g + 15 of all three buffers.
template <bool JOIN, u32 OP, bool GUARD>
__device__ __forceinline__ void rcx_base_flat_step(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst, u64 first, u64 total, u32 tid)
{
    constexpr u32 K = RCX_BASE_U4 / 2;
    u32 w[K][4], b[K][4];
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u64 g = first + j * RCX_BASE_THREADS + tid;
        if (!GUARD || g < total) {
            rcx_load16_any(src + 16ull * g, w[j]);
            rcx_load16_any(ref + 16ull * g, b[j]);
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        const u64 g = first + j * RCX_BASE_THREADS + tid;
        if (!GUARD || g < total) {
            u32 o[4];
            rcx_base_unit<1, OP, JOIN>(w[j], b[j], o);
            rcx_store16<true>(dst + 16ull * g, U4{o[0], o[1], o[2], o[3]});
        }
    }
}

// ===========================================================================
// nfull = n / (W * block), the whole superblocks, as in rcx_planes_k (W = 1: not used, nor is block).
// ===========================================================================
template <u32 W, bool JOIN, u32 OP>
__global__ __launch_bounds__(RCX_BASE_THREADS) void rcx_base_k(const u8* __restrict__ src, const u8* __restrict__ ref, u8* __restrict__ dst, u64 n, u32 block,
                                                               u64 nfull)
{
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "width 1, 2, 4 or 8");
    constexpr u32 STEP = RCX_BASE_ROWS(W) * RCX_BASE_THREADS; // units a workgroup takes at a time
    const u32 tid = threadIdx.x;
    if constexpr (W == 1) {
        const u64 total = n >> 4;
        for (u64 first = (u64)blockIdx.x * STEP; first < total; first += (u64)gridDim.x * STEP) {
            if (first + STEP <= total) rcx_base_flat_step<JOIN, OP, false>(src, ref, dst, first, total, tid);
            else rcx_base_flat_step<JOIN, OP, true>(src, ref, dst, first, total, tid);
        }
        const u64 i = (total << 4) + tid; // the last n % 16 bytes: workgroup 0, one byte a lane
        if (blockIdx.x == 0 && i < n) dst[i] = (u8)rcx_base_elem<1, OP, JOIN>(src[i], ref[i]);
    } else {
        typedef typename RcxElem<W>::T T;
        const u64 super = (u64)W * block;                          // bytes of a whole superblock
        const u32 r_last = (u32)(n - nfull * super);               // bytes of the ragged last one, < W * block <= 2^27
        const u32 m_last = r_last / W;
        const u32 units = block >> 4, units_last = m_last >> 4;    // whole units of a whole superblock (>= 1), of the last one
        const u64 total = nfull * units + units_last;

        for (u64 first = (u64)blockIdx.x * STEP; first < total; first += (u64)gridDim.x * STEP) {
            if (first + STEP <= total) rcx_base_step<W, JOIN, OP, false>(src, ref, dst, first, total, units, nfull, block, m_last, tid);
            else rcx_base_step<W, JOIN, OP, true>(src, ref, dst, first, total, units, nfull, block, m_last, tid);
        }

        // What is left of every superblock behind its whole units, one byte a lane: (m % 16) elements -- the lane makes the
        // whole element and writes its one byte of it -- then R % W tail bytes, which keep the source's values.
        const u32 rest = (block & 15u) * W;                        // of a whole superblock (0 for blocks that are multiples of 16)
        const u32 rest_last = r_last - units_last * (16u * W);     // of the last one, < 17 * W
        const u64 rest_whole = nfull * rest, rest_total = rest_whole + rest_last;
        for (u64 t = (u64)blockIdx.x * RCX_BASE_THREADS + tid; t < rest_total; t += (u64)gridDim.x * RCX_BASE_THREADS) {
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
                const u64 element = at + (u64)e * W;
                T x = 0;
                if (JOIN) {
#pragma unroll
                    for (u32 q = 0; q < W; ++q) x |= (T)src[at + (u64)q * mm + e] << (8u * q);
                } else {
                    x = rcx_load_elem<W>(src + element);
                }
                const u64 v = rcx_base_elem<W, OP, JOIN>(x, rcx_load_elem<W>(ref + element));
                dst[JOIN ? element + p : at + (u64)p * mm + e] = (u8)(v >> (8u * p));
            } else {
                const u64 i = at + (u64)mm * W + (j - in_elements);
                dst[i] = src[i];
            }
        }
    }
}

#endif // !RCX_HOST_SIM
