// rcx_predict.hpp -- the delta predictor for typed integers (include/rcx_predict.h), fused with the byte-plane filter of
// rcx_planes.hpp: split = difference of neighbouring elements (and zigzag), then the planes; join = the planes put together,
// the zigzag undone, then an inclusive prefix sum per superblock.  Superblocks, units and the plane layout are those of
// rcx_planes.hpp; the predictor restarts in every superblock.  All arithmetic is modulo 2^(8W).
//
// Forward is rcx_planes_k<W, false, PRED> of rcx_planes.hpp, which also has the element type and the forward arithmetic
// (RcxElem, rcx_zigzag, rcx_elem_get, rcx_elems_put, rcx_predict_unit, rcx_load_elem).  This file holds what only the
// inverse uses: rcx_unzigzag, the two halves of a unit's scan, rcx_store_elem, the wave scan and the kernel.
//
// Inverse, rcx_predict_join_k<W, ZIGZAG>: ONE WAVE OWNS WHOLE SUPERBLOCKS and walks each one TILE by tile, carrying the
// running element in a register.  THE TILE IS 64 LANES x ONE UNIT = 1024 ELEMENTS (a workgroup is one wave).  Per tile:
// W 16-byte loads a lane (the planes), transpose to elements (rcx_planes_unit), un-zigzag, a serial inclusive scan of the
// lane's 16 elements in registers, an inclusive scan of the wave's 64 lane totals with six __shfl_up steps (two moves a
// step for W = 8, where the sum is a 64-bit add: add with carry), then element + (sum of the lanes in front) + carry, W
// 16-byte stores.  The next tile's loads are issued before the current tile's scan: while the two rows behind a tile are
// whole the loop takes two tiles a turn with two register sets and no branch between its loads and stores (the compiler's
// wait counts then run down load by load, and it has both tiles' loads in flight before the first scan); the last rows
// of a superblock go through a loop with the bounds tests, which loads the next row, or the first row of the wave's next
// superblock, first.  Lanes past the superblock's last unit hold zeros and add nothing, so a
// superblock of fewer than 64 units (B < 1024) is a tile with idle lanes: one code path for every B, and the rate matters
// at B >= 4096 only.  The last m % 16 elements are the end of the same chain: lane k < m % 16 takes element (m & ~15) + k
// byte by byte from the planes, the same wave scan, the same carry.  The R % W tail bytes are copied.
// No wave ever waits for another: no LDS, no barrier, no flag in memory, no scratch, nothing allocated.
//
// It reads exactly [src, src + n) and writes exactly [dst, dst + n), at any alignment (the byte-addressed accesses of
// rcx_planes.hpp and W-byte ones of the same kind).  No floating point, no inline assembly.
#pragma once

#include "rcx_planes.hpp"

#define RCX_PREDICT_TILE_UNITS 64u // the inverse kernel's tile: one wave, one unit a lane = 1024 elements

// ---- the arithmetic of one unit, inverse: plain functions, also compiled for the host (tests/sim/predict_sim.cpp) -----------
// d = (z >> 1) XOR (0 - (z & 1))
template <u32 W>
RCX_DEV typename RcxElem<W>::T rcx_unzigzag(typename RcxElem<W>::T z)
{
    typedef typename RcxElem<W>::T T;
    return ((T)(z >> 1) ^ (T)((T)0 - (T)(z & 1u))) & rcx_elem_mask<W>();
}

// Inverse, first half: e[k] = the sum of the unit's (un-zigzagged) elements 0 .. k; e[15] is the unit's total.
template <u32 W, bool ZIGZAG>
RCX_DEV void rcx_unpredict_scan(const u32 (&in)[4 * W], typename RcxElem<W>::T (&e)[16])
{
    typedef typename RcxElem<W>::T T;
    T sum = 0;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        const T z = rcx_elem_get<W>(in, k);
        sum = (T)(sum + (ZIGZAG ? rcx_unzigzag<W>(z) : z)) & rcx_elem_mask<W>();
        e[k] = sum;
    }
}

// Inverse, second half: out element k = e[k] + before, `before` the sum of everything in front of the unit.
template <u32 W>
RCX_DEV void rcx_unpredict_finish(const typename RcxElem<W>::T (&e)[16], typename RcxElem<W>::T before, u32 (&out)[4 * W])
{
    typedef typename RcxElem<W>::T T;
    T x[16];
#pragma unroll
    for (u32 k = 0; k < 16; ++k) x[k] = (T)(e[k] + before) & rcx_elem_mask<W>();
    rcx_elems_put<W>(x, out);
}

#if !defined(RCX_HOST_SIM)

// An element to W bytes at any byte address.
template <u32 W>
__device__ __forceinline__ void rcx_store_elem(u8* p, typename RcxElem<W>::T v)
{
    if constexpr (W == 2) reinterpret_cast<RcxAnyAlign<uint16_t>*>(p)->v = (uint16_t)v;
    else if constexpr (W == 4) reinterpret_cast<RcxAnyAlign<u32>*>(p)->v = v;
    else reinterpret_cast<RcxAnyAlign<u64>*>(p)->v = v;
}

// Inclusive sum over the wave's 64 lanes; every lane takes part.
template <class T>
__device__ __forceinline__ T rcx_wave_scan(T x, u32 lane)
{
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const T below = __shfl_up(x, d, 64);
        x += lane >= d ? below : (T)0;
    }
    return x;
}

// A unit's W plane pieces: `planes` = the unit's 16 bytes of plane 0, plane p lies p * m further on.
template <u32 W>
__device__ __forceinline__ void rcx_predict_load_unit(const u8* __restrict__ planes, u32 m, u32 (&w)[4 * W])
{
#pragma unroll
    for (u32 i = 0; i < W; ++i) rcx_load16_any(planes + (u64)i * m, &w[4 * i]);
}

// Row `row` of a superblock (m elements a plane, at byte `at`): lane's unit 64 * row + lane; zeros where the superblock has no
// such unit.
template <u32 W>
__device__ __forceinline__ void rcx_predict_load_row(const u8* __restrict__ src, u64 at, u32 m, u32 row, u32 lane, u32 (&w)[4 * W])
{
    const u32 u = row * RCX_PREDICT_TILE_UNITS + lane;
    if (u < (m >> 4)) {
        rcx_predict_load_unit<W>(src + at + 16ull * u, m, w);
    } else {
#pragma unroll
        for (u32 i = 0; i < 4 * W; ++i) w[i] = 0;
    }
}

// One tile: w = the lane's unit as planes (zeros in a lane without one), `elements` where its 16 elements go, `carry` the
// element in front of the tile, afterwards the tile's last one.
template <u32 W, bool ZIGZAG>
__device__ __forceinline__ void rcx_predict_join_tile(const u32 (&w)[4 * W], u8* elements, bool exists, typename RcxElem<W>::T& carry, u32 lane)
{
    typedef typename RcxElem<W>::T T;
    u32 joined[4 * W], out[4 * W];
    T e[16];
    rcx_planes_unit<W, true>(w, joined);
    rcx_unpredict_scan<W, ZIGZAG>(joined, e);
    const T upto = rcx_wave_scan<T>(e[15], lane); // the totals of lanes 0 .. lane
    rcx_unpredict_finish<W>(e, (T)(upto - e[15] + carry), out);
    if (exists) {
#pragma unroll
        for (u32 i = 0; i < W; ++i) rcx_store16<true>(elements + 16ull * i, U4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]});
    }
    carry = (T)(carry + __shfl(upto, 63, 64)) & rcx_elem_mask<W>();
}

template <u32 W, bool ZIGZAG>
__global__ __launch_bounds__(RCX_PREDICT_TILE_UNITS) void rcx_predict_join_k(const u8* __restrict__ src, u8* __restrict__ dst, u64 n, u32 block, u64 nfull)
{
    typedef typename RcxElem<W>::T T;
    constexpr u32 ROW = RCX_PREDICT_TILE_UNITS * 16u;          // plane bytes (= elements) of a tile
    const u64 super = (u64)W * block;
    const u32 r_last = (u32)(n - nfull * super);               // bytes of the ragged last superblock, < W * block <= 2^27
    const u32 m_last = r_last / W;
    const u64 nsuper = nfull + (r_last ? 1u : 0u);
    const u32 lane = threadIdx.x;

    u32 cur[4 * W], nxt[4 * W];
#pragma unroll
    for (u32 i = 0; i < 4 * W; ++i) cur[i] = nxt[i] = 0;
    bool have = false; // cur already holds row 0 of the superblock about to begin

    for (u64 s = blockIdx.x; s < nsuper; s += gridDim.x) {
        const u64 at = s * super;
        const u32 m = s < nfull ? block : m_last;
        const u32 units = m >> 4, rows = (units + RCX_PREDICT_TILE_UNITS - 1) / RCX_PREDICT_TILE_UNITS;
        const u32 full = units / RCX_PREDICT_TILE_UNITS;       // rows in which every lane has a unit
        T carry = 0;                                            // the predictor restarts with the superblock
        if (rows && !have) rcx_predict_load_row<W>(src, at, m, 0, lane, cur);
        have = false;
        u32 row = 0;
        // Two tiles a turn while the two rows behind them are whole: no branch between the loads and the stores, the two
        // register sets take turns, and each tile's loads are issued before the scan of the tile in front of it.
        const u8* planes = src + at + 16ull * lane;             // of the lane's unit in row 0
        u8* elements = dst + at + (u64)lane * (16u * W);
        for (; row + 2 < full; row += 2) {
            rcx_predict_load_unit<W>(planes + (u64)(row + 1) * ROW, m, nxt);
            rcx_predict_join_tile<W, ZIGZAG>(cur, elements + (u64)row * (ROW * W), true, carry, lane);
            rcx_predict_load_unit<W>(planes + (u64)(row + 2) * ROW, m, cur);
            rcx_predict_join_tile<W, ZIGZAG>(nxt, elements + (u64)(row + 1) * (ROW * W), true, carry, lane);
        }
        // The superblock's last rows, with the tests: the next row, or row 0 of this wave's next superblock, is loaded first.
        for (; row < rows; ++row) {
            if (row + 1 < rows) {
                rcx_predict_load_row<W>(src, at, m, row + 1, lane, nxt);
            } else if (s + gridDim.x < nsuper) {
                const u64 s2 = s + gridDim.x;
                const u32 m2 = s2 < nfull ? block : m_last;
                if (m2 >= 16u) {
                    rcx_predict_load_row<W>(src, s2 * super, m2, 0, lane, nxt);
                    have = true;
                }
            }
            const u32 u = row * RCX_PREDICT_TILE_UNITS + lane;
            rcx_predict_join_tile<W, ZIGZAG>(cur, dst + at + (u64)u * (16u * W), u < units, carry, lane);
#pragma unroll
            for (u32 i = 0; i < 4 * W; ++i) cur[i] = nxt[i];
        }
        // the last m % 16 elements: the end of the same chain, one element a lane
        const u32 e0 = m & ~15u, left = m - e0;
        if (left) { // the same in every lane
            T z = 0;
            if (lane < left) {
#pragma unroll
                for (u32 p = 0; p < W; ++p) z |= (T)src[at + (u64)p * m + e0 + lane] << (8u * p);
            }
            const T upto = rcx_wave_scan<T>(ZIGZAG ? rcx_unzigzag<W>(z) : z, lane);
            if (lane < left) rcx_store_elem<W>(dst + at + (u64)(e0 + lane) * W, (T)(upto + carry) & rcx_elem_mask<W>());
        }
        // the R % W bytes behind the last whole element (only the ragged last superblock has any)
        const u32 bytes = s < nfull ? (u32)super : r_last;
        if (lane < bytes - m * W) dst[at + (u64)m * W + lane] = src[at + (u64)m * W + lane];
    }
}

#endif // !RCX_HOST_SIM
