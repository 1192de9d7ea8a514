// rcx_crc.hpp -- CRC-32 of every work entry (block or item) on the GPU, stored or compared with an expected value.
//
// The checksum is zlib's crc32: polynomial 0xEDB88320 (reflected), init and final XOR 0xFFFFFFFF, crc32("") == 0.
//
// A CRC register is a polynomial over GF(2) modulo P, bit 31 = x^0 (reflected).  Taking in a byte c is
// s' = (s ^ c) * x^8 mod P, a little-endian dword w is s' = (s ^ w) * x^32 mod P, and k zero bytes behind that multiply
// by x^(8k): everything here is a multiplication by a constant power of x, and the whole is linear in the data.
//
// One wave per entry.  The entry's aligned dwords (its BODY, D of them) are read row by row -- 64 lanes x one dword = 256
// bytes, coalesced -- and lane l folds only its own dwords l, l + 64, ...: per row x = state ^ word and
// state = x * x^2048, looked up in four 256-entry tables (S_j[b] = the byte b at position j of x, times x^2048: the
// ordinary slicing tables for a stride of 256 bytes instead of 4).  A lane's LAST dword is instead advanced over its own
// distance to the end of the body, 4 .. 256 bytes: one multiplication by x^(32 * dist) per lane and entry
// (rcx_crc_mul, 32 shift-and-xor steps; the powers are a table of 64).  The lanes' states are then XOR-reduced over the
// wave.  The register that enters the body -- the init value taken through the up to 3 head bytes in front of the first
// aligned dword -- is lane 0's start state, so it is carried over the body with lane 0's first dword; the up to 3 tail
// bytes behind the body go through the plain byte table.  A partial last row is part of the body: lanes below D % 64
// have their last dword there, the others in the row before.
//
// LDS: the byte table, the four stride tables and the 65 powers, 5380 bytes per workgroup of four waves, copied from
// constexpr tables in device memory when the workgroup starts; a workgroup then takes entries in a grid-stride loop.
// The table indices depend on the data: ds_read_b32 serves 32 lanes per LDS cycle from 32 banks, so a row's four
// look-ups conflict at random (DESIGN.md section 10 has what was measured).  No floating point, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>

#include "rcx_geom.hpp"

#define RCX_CRC_POLY 0xEDB88320u
#define RCX_CRC_WAVES 4     // waves (entries in flight) per workgroup
#define RCX_CRC_T_BYTE 0    // tab[b]: b * x^8
#define RCX_CRC_T_ROW 256   // tab[256 + 256 * j + b]: (b << 8j) * x^2048
#define RCX_CRC_T_POW 1280  // tab[1280 + k]: x^(32k), k = 0 .. 64
#define RCX_CRC_T_WORDS 1345

// a * b mod P
__host__ __device__ constexpr u32 rcx_crc_mul(u32 a, u32 b)
{
    u32 p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (RCX_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

struct RcxCrcTables {
    u32 w[RCX_CRC_T_WORDS];
};

constexpr RcxCrcTables rcx_crc_make_tables()
{
    RcxCrcTables t{};
    u32* pw = t.w + RCX_CRC_T_POW;
    pw[0] = 0x80000000u; // x^0
    for (int k = 1; k <= 64; ++k) pw[k] = rcx_crc_mul(pw[k - 1], RCX_CRC_POLY); // x^32 mod P = P without its x^32 term
    // a table is linear in its index: eight products per table, the other entries are their sums
    for (int tab = 0; tab < 5; ++tab) {
        u32* e = t.w + 256 * tab;
        for (int bit = 0; bit < 8; ++bit)
            e[1 << bit] = tab == 0 ? rcx_crc_mul(1u << bit, 0x00800000u /* x^8 */) : rcx_crc_mul((1u << bit) << (8 * (tab - 1)), pw[64]);
        for (int b = 1; b < 256; ++b) e[b] = e[b & (b - 1)] ^ e[b & (0 - b)];
    }
    return t;
}

static __device__ const RcxCrcTables rcx_crc_tables = rcx_crc_make_tables();

__device__ __forceinline__ u32 rcx_crc_byte(const u32* tab, u32 s, u32 c) { return tab[RCX_CRC_T_BYTE + ((s ^ c) & 255u)] ^ (s >> 8); }

// x * x^2048: the register, one dword taken in, 252 bytes further on
__device__ __forceinline__ u32 rcx_crc_row(const u32* tab, u32 x)
{
    return tab[RCX_CRC_T_ROW + (x & 255u)] ^ tab[RCX_CRC_T_ROW + 256 + ((x >> 8) & 255u)] ^ tab[RCX_CRC_T_ROW + 512 + ((x >> 16) & 255u)] ^
           tab[RCX_CRC_T_ROW + 768 + (x >> 24)];
}

// The CRC-32 of the len bytes at p (any alignment), computed by one wave; every lane returns it.  Reads [p, p + len) only.
__device__ __forceinline__ u32 rcx_crc_wave(const u32* tab, const u8* p, u32 len, u32 lane)
{
    u32 head = (u32)((0 - reinterpret_cast<uintptr_t>(p)) & 3u);
    if (head > len) head = len;
    u32 s = 0xFFFFFFFFu;
    for (u32 i = 0; i < head; ++i) s = rcx_crc_byte(tab, s, p[i]);
    const u32 D = (len - head) >> 2; // the body's dwords, < 2^22
    if (D) {
        const u32* q = reinterpret_cast<const u32*>(p + head) + lane;
        const u32 full = D >> 6, k = D & 63u;
        const u32 steps = full ? full - 1 : 0; // rows in which every lane has a later dword
        u32 st = lane == 0 ? s : 0u;
        u32 r = 0;
        if (steps >= 8) { // eight rows in flight while the eight before them are folded
            u32 cur[8], nxt[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) cur[j] = q[(r + j) * 64u];
            for (; r + 16 <= steps; r += 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) nxt[j] = q[(r + 8 + j) * 64u];
#pragma unroll
                for (int j = 0; j < 8; ++j) st = rcx_crc_row(tab, st ^ cur[j]);
#pragma unroll
                for (int j = 0; j < 8; ++j) cur[j] = nxt[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) st = rcx_crc_row(tab, st ^ cur[j]);
            r += 8;
        }
        for (; r < steps; ++r) st = rcx_crc_row(tab, st ^ q[r * 64u]);
        // the last whole row, then the partial one: a lane's last dword goes its own distance to the end of the body
        u32 x = 0;
        if (full) {
            x = st ^ q[(full - 1) * 64u];
            if (lane < k) st = rcx_crc_row(tab, x);
        }
        if (lane < k) x = st ^ q[full * 64u];
        const u32 dist = lane < k ? k - lane : k + 64u - lane; // in dwords, 1 .. 64
        st = (full || lane < k) ? rcx_crc_mul(x, tab[RCX_CRC_T_POW + dist]) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) st ^= (u32)__shfl_xor((int)st, o, 64);
        s = st;
    }
    for (u32 i = head + 4u * D; i < len; ++i) s = rcx_crc_byte(tab, s, p[i]);
    return ~s;
}

// ===========================================================================
// CRC-32 of every work entry.  VERIFY = false: crc[id] = the entry's CRC.  VERIFY = true: nothing is written but the
// latch -- an entry whose CRC differs from expected[id] is flagged RCX_ST_CORRUPT with its id.
// Blocks: id = the block; items: id = the item (the tables are in work order), an item of length 0 has CRC 0.
// ===========================================================================
template <bool VERIFY, class G = RcxBlocks>
__global__ __launch_bounds__(64 * RCX_CRC_WAVES) void rcx_crc32_k(const u8* __restrict__ src, u64 n, u32 block, u64 nblocks, u32* __restrict__ crc,
                                                                    const u32* __restrict__ expected, u32* status, const G g = G())
{
    __shared__ u32 tab[RCX_CRC_T_WORDS];
    for (u32 i = threadIdx.x; i < RCX_CRC_T_WORDS; i += 64 * RCX_CRC_WAVES) tab[i] = rcx_crc_tables.w[i];
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (u64 blk = (u64)blockIdx.x * RCX_CRC_WAVES + wave; blk < nblocks; blk += (u64)gridDim.x * RCX_CRC_WAVES) {
        RCX_ENTRY(g, blk, nblocks, n, block);
        (void)live;
        const u32 value = rcx_crc_wave(tab, src + at, len, lane);
        if (lane == 0) {
            const u64 id = rcx_id(g, blk);
            if (VERIFY) {
                if (value != expected[id]) rcx_flag(status, RCX_ST_CORRUPT, id);
            } else {
                crc[id] = value;
            }
        }
    }
}
