// rcx_predict.hpp -- the delta predictor for typed integers (include/rcx_predict.h), fused with the byte-plane filter of
// rcx_planes.hpp: split = difference of neighbouring elements (and zigzag), then the planes; join = the planes put together,
// the zigzag undone, then an inclusive prefix sum per superblock.  Superblocks, units and the plane layout are those of
// rcx_planes.hpp; the predictor restarts in every superblock.  All arithmetic is modulo 2^(8W).
//
// Forward, rcx_predict_split_k<W, ZIGZAG>: the shape of rcx_planes_k's split -- a lane's unit is 16 elements, a fixed grid
// loops, a workgroup takes RCX_PLANES_U4 / W rows of 256 units at a time with all their loads in flight, a guarded last
// step, a byte-wise rest.  The difference is taken in registers between load and transpose; the element in front of a
// unit comes from one more W-byte load at (the unit's first element - W), a line the neighbouring lane fetches anyway, and
// is 0 for the first unit of a superblock.  A rest byte's lane loads its element and the one in front.  No LDS.
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
// Both read exactly [src, src + n) and write exactly [dst, dst + n), at any alignment (the byte-addressed accesses of
// rcx_planes.hpp and W-byte ones of the same kind).  No floating point, no inline assembly.
#pragma once

#include "rcx_planes.hpp"

#define RCX_PREDICT_TILE_UNITS 64u // the inverse kernel's tile: one wave, one unit a lane = 1024 elements

// ---- the arithmetic of one unit: plain functions, also compiled for the host (tests/sim/predict_sim.cpp) -------------------
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

// d = (z >> 1) XOR (0 - (z & 1))
template <u32 W>
RCX_DEV typename RcxElem<W>::T rcx_unzigzag(typename RcxElem<W>::T z)
{
    typedef typename RcxElem<W>::T T;
    return ((T)(z >> 1) ^ (T)((T)0 - (T)(z & 1u))) & rcx_elem_mask<W>();
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

// W bytes at any byte address as an element, and back.
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

template <u32 W>
__device__ __forceinline__ void rcx_store_elem(u8* p, typename RcxElem<W>::T v)
{
    if constexpr (W == 2) reinterpret_cast<RcxAnyAlign<uint16_t>*>(p)->v = (uint16_t)v;
    else if constexpr (W == 4) reinterpret_cast<RcxAnyAlign<u32>*>(p)->v = v;
    else reinterpret_cast<RcxAnyAlign<u64>*>(p)->v = v;
}

// ===========================================================================
// Forward.  rcx_planes_step's split with the difference between load and transpose.
// ===========================================================================
template <u32 W, bool ZIGZAG, bool GUARD>
__device__ __forceinline__ void rcx_predict_split_step(const u8* __restrict__ src, u8* __restrict__ dst, u64 base, u64 total, u32 units, u64 nfull,
                                                       u32 block, u32 m_last, u32 tid)
{
    typedef typename RcxElem<W>::T T;
    constexpr u32 K = RCX_PLANES_U4 / W;
    const u64 s0 = base / units;
    const u32 u0 = (u32)(base - s0 * units);
    u32 w[K][4 * W];
    T prev[K];
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
        const u64 elements = at + (u64)u * (16u * W);
        to[j] = at + 16ull * u; // plane p: + p * m
        prev[j] = 0;            // the predictor restarts with the superblock
        if (!GUARD || base + j * RCX_PLANES_THREADS + tid < total) {
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_load16_any(src + elements + 16ull * i, &w[j][4 * i]);
            if (u) prev[j] = rcx_load_elem<W>(src + elements - W);
        }
    }
#pragma unroll
    for (u32 j = 0; j < K; ++j) {
        if (!GUARD || base + j * RCX_PLANES_THREADS + tid < total) {
            u32 d[4 * W], o[4 * W];
            rcx_predict_unit<W, ZIGZAG>(w[j], prev[j], d);
            rcx_planes_unit<W, false>(d, o);
#pragma unroll
            for (u32 i = 0; i < W; ++i) rcx_store16<true>(dst + to[j] + (u64)i * m[j], U4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]});
        }
    }
}

template <u32 W, bool ZIGZAG>
__global__ __launch_bounds__(RCX_PLANES_THREADS) void rcx_predict_split_k(const u8* __restrict__ src, u8* __restrict__ dst, u64 n, u32 block, u64 nfull)
{
    typedef typename RcxElem<W>::T T;
    constexpr u32 STEP = RCX_PLANES_U4 / W * RCX_PLANES_THREADS; // units a workgroup takes at a time
    const u64 super = (u64)W * block;                            // bytes of a whole superblock
    const u32 r_last = (u32)(n - nfull * super);                 // bytes of the ragged last one, < W * block <= 2^27
    const u32 m_last = r_last / W;
    const u32 units = block >> 4, units_last = m_last >> 4;      // whole units of a whole superblock (>= 1), of the last one
    const u64 total = nfull * units + units_last;
    const u32 tid = threadIdx.x;

    for (u64 base = (u64)blockIdx.x * STEP; base < total; base += (u64)gridDim.x * STEP) {
        if (base + STEP <= total) rcx_predict_split_step<W, ZIGZAG, false>(src, dst, base, total, units, nfull, block, m_last, tid);
        else rcx_predict_split_step<W, ZIGZAG, true>(src, dst, base, total, units, nfull, block, m_last, tid);
    }

    // What is left of every superblock behind its whole units, one byte a lane: (m % 16) elements, each against the element
    // in front of it, then R % W tail bytes as they are.
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
            const u8* element = src + at + (u64)e * W;
            const T here = rcx_load_elem<W>(element), front = e ? rcx_load_elem<W>(element - W) : (T)0;
            const T d = (T)(here - front) & rcx_elem_mask<W>();
            dst[at + (u64)p * mm + e] = (u8)((ZIGZAG ? rcx_zigzag<W>(d) : d) >> (8u * p));
        } else {
            const u64 i = at + (u64)mm * W + (j - in_elements);
            dst[i] = src[i];
        }
    }
}

// ===========================================================================
// Inverse.
// ===========================================================================
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
