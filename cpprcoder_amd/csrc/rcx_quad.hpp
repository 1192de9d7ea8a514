// rcx_quad.hpp -- what a "4 lanes per block" decoder is made of, and the adaptive one itself:
//   the cross-lane (DPP) helpers, the LDS layout of a wave's 16 blocks, the lane's seat in it (QuadSeat), the stream
//   lookup and its failing exit, QuadInput (the block's compressed stream through an LDS ring), the pieces of
//   instruction text the three symbol sequences share, the parked 64-byte output, the closing redo marks
//   rcx_dec_quad_k   adaptive decode, 4 lanes per block (16 blocks per wave)
// rcx_dec_static_quad_k (rcx_static.hpp) and rcx_dec_rans1_quad_k (rcx_rans.hpp) are built on the same frame.
#pragma once
// included by rcx_kernels.hpp (uses rcx_flag, rcx_wave_max from there)

template <int CTRL>
__device__ __forceinline__ u32 rcx_dpp(u32 x)
{
    return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
// sum over the 8 lanes of an octet, result in all of them
__device__ __forceinline__ u32 rcx_oct_sum(u32 x)
{
    x += rcx_dpp<0xB1>(x);  // quad_perm [1,0,3,2]
    x += rcx_dpp<0x4E>(x);  // quad_perm [2,3,0,1]
    x += rcx_dpp<0x141>(x); // row_half_mirror: lane i <-> 7-i
    return x;
}
// exclusive prefix over the 8 lanes of an octet (lane j gets x_0 + ... + x_{j-1})
__device__ __forceinline__ u32 rcx_oct_excl_scan(u32 x, u32 m1, u32 m2, u32 m4)
{
    u32 tot = x, pre = 0, o;
    o = rcx_dpp<0xB1>(tot);
    pre += o & m1;
    tot += o;
    o = rcx_dpp<0x4E>(tot);
    pre += o & m2;
    tot += o;
    o = rcx_dpp<0x141>(tot); // the other quad's total
    pre += o & m4;
    return pre;
}

// ===========================================================================
// Decode, 4 lanes per block ("quad"): 16 blocks per wave, 1024 waves for 1 GiB of 64 KiB
// blocks = one wave per SIMD.  A lone wave issues one instruction -- vector, scalar, s_nop or
// s_waitcnt alike -- every 4 cycles and hides no latency (tools/diag/ubench.hip), so the kernel is
// written for the fewest instructions per symbol of any kind, and for work between the one
// dependent LDS read and its use.
//
// Model (cpprcoder.h:1094-1243): the alphabet is split 16 nodes x 16 symbols.  Lane j of the
// block's quad keeps in REGISTERS U1..U4 = the counts of all symbols below node 4j+1, ..., 4j+4
// (absolute cumulative sums: the upper bounds of its four nodes; U4 of the last lane is the
// total) -- negated, nU_k = -U_k, see below; the 256 counts live in LDS, node n as 64 contiguous
// bytes of which lane j reads counts 4j..4j+3 (one ds_read_b128).
//
// find() (cpprcoder.h:1220-1242) in the scaled domain (see DecLane), without selects:
//   x_k = low - U_k*t wraps past zero exactly for the bounds above low, so
//     * the number of bounds that do NOT borrow, summed over the quad, is the node index,
//     * the unsigned minimum of low and all x_k over the quad is low - cum(node)*t;
//   round 1 takes both from one v_mad_i64_i32 per bound, {low, 0} + nU_k*t: x_k is its low word, the borrow -- 0 or
//   -1 -- its high word h_k, and the model update (+1 on every bound above the symbol's node) is nU_k += h_k.
//   h_k is 0 or -1 on ANY input: t = floor(r / (256 + i)) for whatever 32-bit r the renormalised range is (the divisor
//   entries are exact, rcx_divtab.hpp; a wrapped r + inc gives t = 0), and U_k <= 256 + i as long as every h so far was
//   0 or -1, so U_k*t <= r < 2^32 and low - U_k*t > -2^32: by induction the node index is 0 .. 16 and a symbol raises a
//   bound by at most one, however damaged the stream;
//   round 2 is the same over the node's 16 counts, and the unsigned maximum of the x over the
//   quad is the (wrapped) distance to the smallest bound above, so the new range count*t is
//   min - max (mod 2^32): cum(c+1)*t - cum(c)*t, no multiply, no select of the count.
//   The counts are negated in LDS too (-1 at the start).  With P = minus the counts of the node's symbols in lower lanes,
//   D = {rem, 0} + P*t and Y_k = Y_(k-1) + l_k*t (Y_0 = D, l_k the lane's k-th negated count) are five more
//   v_mad_i64_i32: the low words are the y of old, the high words their borrows.  For a node row every partial sum Q is
//   0 <= Q <= the node's total and total*t <= range < 2^32, so in the lane that owns the symbol and in those below it
//   (D >= 0) every high word is 0 or -1: the symbol is the lane's last one plus three of them, and ~h_D & h_e is the
//   owner word, -1 in the owning lane and 0 elsewhere (above it D < 0, h_e is -1 or -2 and h_D = -1 masks it).  That word
//   is what ds_add puts on the count and what masks the output byte.  The scratch row's "counts" are arbitrary, and so are
//   the symbol and the owner word then: the symbol reaches memory only as bits 2 and 3 of its fourfold, inserted into
//   the 16-byte aligned address of the lane's 16 bytes of the row round 1 chose (0 .. 16), and as an output byte of a
//   block that is marked and decoded again, the owner word only as the ds_add's operand into that scratch row (DESIGN
//   3.4, rounds 7 and 9).
// A target at or past the total (corrupt input only) leaves no borrow in round 1 and "node 16",
// whose counts are a scratch area behind the block's table.  Such a block is detected, not
// decoded: it is marked in `redo` and decoded again by rcx_dec_adaptive_k, which has the
// reference's fall-through for that case.
//
// Input: no bit window.  The position in the stream is a bit offset `bp8`; the two ring dwords
// around it are read right after each renormalisation (for the NEXT symbol, so their latency is
// never waited for) and the next four bytes are one v_alignbit + one byte swap away.
// ===========================================================================
#define RCX_QUAD_BLOCKS 16
// LDS of one wave: four 4352-byte table groups | sixteen 144-byte input rings.
//   A ds_read_b128 is served in four groups of 16 lanes -- quads {0,3,5,6}, {1,2,4,7}, {8,11,13,14},
//   {9,10,12,15} -- one LDS cycle each if the group's four 64-byte reads fall into four different quarters
//   of the 256-byte bank row (MI355X_MICROARCH.md, LDS).  So the four blocks of such a group share a table
//   group: row n (256 bytes) holds node n of all four, block s in quarter s; whatever nodes the four quads
//   ask for, they read different quarters.  (One table per block: 16 of the 36 LDS cycles per symbol were
//   bank conflicts.)  Row 16 is scratch ("node 16"): per block three 16-byte groups of decoded output
//   waiting for the fourth (the loops of 16 symbols; the adaptive decoder's pass of 64 keeps its four groups in
//   registers and puts nothing there), then 16 bytes where skipped ring writes go.
//   A ring is 32 dwords + slot 32 (repeats slot 0) + 12 spare bytes; 36 dwords apart, the rings of the 8
//   quads of a half-wave start 4 banks apart.
#define RCX_QUAD_GROUP_BYTES 4352
#define RCX_QUAD_RING_BYTES 144
#define RCX_QUAD_LDS_BYTES (4 * RCX_QUAD_GROUP_BYTES + RCX_QUAD_BLOCKS * RCX_QUAD_RING_BYTES) /* 19.25 KiB: two 4-wave workgroups per CU */

// LDS addresses computed inside the instruction sequences come back as 32-bit offsets
typedef u32 RcxV4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) RcxV4 RcxLdsV4;
typedef __attribute__((address_space(3))) u32 RcxLdsU32;
typedef RcxV4 RcxDivQv;          // a staged divisor as four dwords: mul, shift (| total << 5), addend low, addend high
typedef RcxLdsV4 RcxLdsDivQ;

// The quad decoder's divisors (rcx_api.hip builds them next to the DivEntry table): per 16 symbols -- entries
// 16G .. 16G+15 -- 32 dwords at 32G: the 16 multipliers, then 16 increments, 1 where the entry's addend is its
// multiplier (round-down magic, powers of two) and 0 where it is 0 (rcx_divtab.hpp: there is no other case).  For a
// range r < 2^32 - 1, (r * mul + add) >> 32 == mulhi(r + inc, mul).  The shift is floor(log2(total)), the same for
// all 16 entries of such a group (the powers of two from 256 up are multiples of 16), so it is not stored.
#define RCX_QUAD_DIVQ_DW 32

__device__ __forceinline__ u32 rcx_quad_sum(u32 x)
{
    x += rcx_dpp<0xB1>(x); // quad_perm [1,0,3,2]
    x += rcx_dpp<0x4E>(x); // quad_perm [2,3,0,1]
    return x;
}
__device__ __forceinline__ u32 rcx_umin(u32 a, u32 b) { return a < b ? a : b; }
__device__ __forceinline__ u32 rcx_umax(u32 a, u32 b) { return a > b ? a : b; }
__device__ __forceinline__ u32 rcx_quad_min(u32 x)
{
    x = rcx_umin(x, rcx_dpp<0xB1>(x));
    x = rcx_umin(x, rcx_dpp<0x4E>(x));
    return x;
}
__device__ __forceinline__ u32 rcx_quad_max(u32 x)
{
    x = rcx_umax(x, rcx_dpp<0xB1>(x));
    x = rcx_umax(x, rcx_dpp<0x4E>(x));
    return x;
}
__device__ __forceinline__ u32 rcx_quad_or(u32 x)
{
    x |= rcx_dpp<0xB1>(x);
    x |= rcx_dpp<0x4E>(x);
    return x;
}
__device__ __forceinline__ u32 rcx_quad_excl_scan(u32 x, u32 m1, u32 m2)
{
    u32 o = rcx_dpp<0xB1>(x);
    u32 pre = o & m1;
    const u32 tot = x + o;
    o = rcx_dpp<0x4E>(tot);
    pre += o & m2;
    return pre;
}

// The compressed stream of one block as its quad reads it (all 4 lanes hold the same state and
// store the same values).
// Ring: dword d of the stream (counted from `origin`, the 16-byte aligned address at or below the
// first payload byte) lives in ring[d % 32]; ring[32] repeats ring[0] so that the pair (d, d+1)
// is always one ds_read2_b32.  Every 16 symbols (which consume at most 12 dwords) topup() moves the 16-byte
// piece it requested the time before into the ring and requests the next one -- unconditionally: a piece the
// ring has no room for is written to the scratch area instead and asked for again.  One piece per 16 symbols is
// one byte per symbol: a quad that needs more (expanding data for a while, or a burst of improbable symbols)
// falls behind and is refilled synchronously, up to 24 dwords ahead, on a cold branch.
#if !defined(RCX_TOPUP_PIECES)
#define RCX_TOPUP_PIECES 1 /* 16-byte pieces requested per top-up on the fast path (2: 1 % slower on 1.0-ratio data) */
#endif
struct QuadInput {
    u32 low, range;
    u32 bp8;        // bits of the stream consumed, counted from `origin`
    u32 w0, w1;     // ring dwords (bp8 >> 5) and (bp8 >> 5) + 1, raw (memory order)
    u32 n4;         // the four stream bytes at bp8, first one on top
    u32* ring;      // this block's ring
    U4* skipped;    // 16 bytes that take the ring writes that are skipped
    u32 wr;         // dwords written to the ring so far
    u32 nfit;       // how many of pendA, pendB (requested at the last top-up) the ring has room for
    U4 pendA, pendB;
    const u8* origin;
    u32 last_off;   // byte offset from origin of the last 16-byte piece that may be loaded
    u32 body8;      // bit offset of the first payload byte (after the 8 header bytes)

    // a piece at or past the end of the stream repeats the stream's last piece (never used by a valid
    // stream; the piece holding the last byte stays inside that byte's page)
    __device__ __forceinline__ U4 load16(u32 off) const
    {
        return *reinterpret_cast<const U4*>(origin + (off < last_off ? off : last_off));
    }
    __device__ __forceinline__ void ring_put(const U4& piece, bool really)
    {
        const u32 slot = wr % RCX_RING_DW; // a multiple of 4: the piece never wraps
        *(really ? reinterpret_cast<U4*>(ring + slot) : skipped) = piece;
        ring[really && slot == 0 ? RCX_RING_DW : RCX_RING_DW + 1] = piece.x;
        wr += really ? 4u : 0u;
    }
    __device__ __forceinline__ void fetch_pair()
    {
        const u32* at = ring + ((bp8 >> 5) % RCX_RING_DW);
        w0 = at[0];
        w1 = at[1];
    }
    // cpprcoder.h:877-896 + :859-870; `s` must hold at least 8 bytes.  Returns the declared size.
    __device__ __forceinline__ u32 begin(const u8* s, const u8* stream_end, u32* block_ring, U4* scratch16)
    {
        skipped = scratch16;
        const u32 declared = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
        low = ((u32)s[4] << 24) | ((u32)s[5] << 16) | ((u32)s[6] << 8) | (u32)s[7];
        range = 0x00FFFFFFu;
        ring = block_ring;
        const u8* body = s + 8;
        origin = body - ((uintptr_t)body & 15);
        last_off = (u32)(stream_end - 1 - origin) & ~15u;
        wr = 0;
        for (u32 r = 0; r < 6; ++r) ring_put(load16(16 * r), true); // prologue: 24 dwords, synchronously
        nfit = 0;
        pendA.x = pendA.y = pendA.z = pendA.w = 0;
        pendB = pendA;
        body8 = 8u * (u32)(body - origin);
        bp8 = body8;
        fetch_pair();
        n4 = rcx_bswap(rcx_funnel_shr(w1, w0, bp8));
        return declared;
    }
    // a lane without a block: reads 16 bytes at the start of the compressed buffer, over and over
    __device__ __forceinline__ void idle(const u8* anywhere, u32* block_ring, U4* scratch16)
    {
        skipped = scratch16;
        low = 0;
        range = 0x01000000u;
        ring = block_ring;
        origin = anywhere - ((uintptr_t)anywhere & 15);
        last_off = 0;
        wr = 24;
        nfit = 0;
        pendA.x = pendA.y = pendA.z = pendA.w = 0;
        pendB = pendA;
        body8 = bp8 = 0;
        w0 = w1 = n4 = 0;
    }
    __device__ __forceinline__ void topup()
    {
        ring_put(pendA, nfit >= 1);
#if RCX_TOPUP_PIECES > 1
        ring_put(pendB, nfit >= 2);
#endif
        const u32 rd = bp8 >> 5; // ring[rd % 32 ...] are unread
        if (rcx_any(wr - rd < 14u)) { // the next 16 symbols may need 12 dwords and the pair after them
            asm volatile("" ::: "memory"); // keep this a branch: taken only on a run of very improbable symbols
            while (__any(wr - rd <= 20u)) ring_put(load16(4 * wr), wr - rd <= 20u);
        }
        const u32 room = (rd + RCX_RING_DW - wr) >> 2;
        nfit = room < (u32)RCX_TOPUP_PIECES ? room : (u32)RCX_TOPUP_PIECES;
        pendA = load16(4 * wr);
#if RCX_TOPUP_PIECES > 1
        pendB = load16(4 * wr + 16);
#endif
    }
    // stream bytes consumed so far, header included (cpprcoder.h:901-903)
    __device__ __forceinline__ u64 taken() const { return 8 + (u64)((bp8 - body8) >> 3); }
};

// The lane's seat in a quad decoder's workgroup of WAVES waves: which block it works on, and where that block's things
// lie in LDS (the layout above).
// quads_used (1, 2, 4, 8 or 16) of the wave's 16 quads carry a block (rcx_api.hip picks it from the block count so that
// every SIMD of the machine has a wave before any wave carries 16 blocks).  The other quads decode the block of quad
// (quad mod quads_used) along with it -- same instructions, well-defined state -- and store nothing.
struct QuadSeat {
    u32 lane, wave; // of the wave, of the workgroup
    u32 quad, j;    // the lane's quad, and its place in it
    bool in_use;    // the quad carries a block of its own
    u64 blk;
    u8* lds;        // the wave's
    u8* mine;       // the block's quarter of its table group: row n at mine + 256 n
    U4* leaves;     // the lane's four entries of node n: leaves[n * 16]
    U4* parked;     // the scratch row ("node 16")
    u32* ring;      // the block's input ring
};
// How a quad decoder opens: declares SEAT, filled from threadIdx, blockIdx, WAVES, QUADS_USED and the workgroup's LDS, and
// the block's `live`, `at`, `len` (RCX_ENTRY).  A macro, and the entry in the middle of it, because these lines come out
// as the same instructions only in this order and in place: filled by a function, or with the entry behind the seat,
// every quad kernel's prologue is scheduled differently and the item kernels' get another instruction.
#define RCX_QUAD_SEAT(SEAT, WAVES, QUADS_USED, LDS_ALL, GEOM, NBLOCKS, N, BLOCK)                                       \
    QuadSeat SEAT;                                                                                                     \
    SEAT.lane = threadIdx.x & 63u;                                                                                     \
    SEAT.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                                      \
    SEAT.lds = (LDS_ALL) + SEAT.wave * RCX_QUAD_LDS_BYTES;                                                             \
    SEAT.j = SEAT.lane & 3u, SEAT.quad = SEAT.lane >> 2;                                                               \
    SEAT.in_use = SEAT.quad < (QUADS_USED);                                                                            \
    SEAT.blk = ((u64)blockIdx.x * (WAVES) + SEAT.wave) * (QUADS_USED) + (SEAT.quad & ((QUADS_USED)-1u));               \
    RCX_ENTRY(GEOM, SEAT.blk, NBLOCKS, N, BLOCK);                                                                      \
    {                                                                                                                  \
        /* table group and quarter of this quad: the quads a ds_read_b128 serves together share a group */             \
        const u32 group = 2u * (SEAT.quad >> 3) + ((0x96u >> (SEAT.quad & 7u)) & 1u), quarter = (SEAT.quad & 7u) >> 1; \
        SEAT.mine = SEAT.lds + group * RCX_QUAD_GROUP_BYTES + quarter * 64;                                            \
        SEAT.leaves = reinterpret_cast<U4*>(SEAT.mine) + SEAT.j;                                                       \
        SEAT.parked = reinterpret_cast<U4*>(SEAT.mine + 16 * 256);                                                     \
        SEAT.ring = reinterpret_cast<u32*>(SEAT.lds + 4 * RCX_QUAD_GROUP_BYTES + SEAT.quad * RCX_QUAD_RING_BYTES);     \
    }

// A block that cannot be decoded (its stream's bounds, its header): the quad's first lane reports it, and the quad goes
// on as one without a block.
#define RCX_QUAD_FAIL(SEAT, GEOM, STATUS)                                                                              \
    {                                                                                                                  \
        if (SEAT.j == 0 && SEAT.in_use) rcx_flag(STATUS, RCX_ST_CORRUPT, rcx_id(GEOM, SEAT.blk));                      \
        live = false;                                                                                                  \
        len = 0;                                                                                                       \
    }
// How the range decoders close: every block of the launch gets its mark in REDO (MARKED: decode it again, one lane per block).
#define RCX_QUAD_MARK_REDO(SEAT, REDO, NBLOCKS, MARKED)                                                                \
    if (leader) (REDO)[SEAT.blk] = (MARKED) ? 1u : 0u;                                                                 \
    else if (SEAT.j == 0 && SEAT.in_use && SEAT.blk < (NBLOCKS)) (REDO)[SEAT.blk] = 0

// The parked output of the range decoders' fast loops.  64 decoded bytes leave as four back-to-back 16-byte stores, so
// that L2 sees whole 64-byte pieces (16-byte pieces 16 symbols apart were written to HBM one by one: 4x WRITE_SIZE).
// Groups 0..2 wait in the block's scratch row PARKED, group 3 in the registers LAST (a U4 that starts as zeroes), and
// the stores are issued right AFTER the next top-up: its s_waitcnt vmcnt for the input pieces would otherwise wait for
// these stores as well.  I0 = the index of a group's first symbol; ANY_ALIGN: rcx_store16.
// (Macros, not a type with three members: with that, the two kernels' loops came out different, 31 instructions longer.)
// behind the top-up in front of group I0: the 64 bytes before it, if it is the first of four
#define RCX_QUAD_PARKED_FLUSH(I0, PARKED, LAST, ANY_ALIGN)                                                             \
    const u32 g = ((I0) >> 4) & 3u;                                                                                    \
    if (g == 0 && (I0) != 0 && leader) {                                                                               \
        u8* o4 = out + ((I0)-64);                                                                                      \
        const U4 p0 = (PARKED)[0], p1 = (PARKED)[1], p2 = (PARKED)[2];                                                 \
        rcx_store16<ANY_ALIGN>(o4, p0);                                                                                \
        rcx_store16<ANY_ALIGN>(o4 + 16, p1);                                                                           \
        rcx_store16<ANY_ALIGN>(o4 + 32, p2);                                                                           \
        rcx_store16<ANY_ALIGN>(o4 + 48, LAST);                                                                         \
    }
// the group's 16 bytes O (the quad's 4 lanes store the same)
#define RCX_QUAD_PARKED_PUT(O, PARKED, LAST)                                                                           \
    if (g == 3) LAST = O;                                                                                              \
    else (PARKED)[g] = O
// behind the loop, which made END bytes: what is still parked, the last 16..64 of them
#define RCX_QUAD_PARKED_END(END, PARKED, LAST, ANY_ALIGN)                                                              \
    if (leader && (END) != 0) {                                                                                        \
        const u32 groups = (((END)-1) >> 4 & 3u) + 1;                                                                  \
        u8* o4 = out + (((END)-1) & ~63u);                                                                             \
        rcx_store16<ANY_ALIGN>(o4, (PARKED)[0]);                                                                       \
        if (groups > 1) rcx_store16<ANY_ALIGN>(o4 + 16, (PARKED)[1]);                                                  \
        if (groups > 2) rcx_store16<ANY_ALIGN>(o4 + 32, (PARKED)[2]);                                                  \
        if (groups > 3) rcx_store16<ANY_ALIGN>(o4 + 48, LAST);                                                         \
    }

// ---------------------------------------------------------------------------
// Pieces of instruction text the symbol sequences of the quad decoders share.  (Why instruction sequences at all:
// rcx_dec_quad_k.)
// ---------------------------------------------------------------------------
#define RCX_QP1 "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define RCX_QP2 "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"

// Round 2 of a symbol over a table that is already cumulative (the static range decoder, rANS): which of the node's 16
// entries -- the lane's four are Q1..Q4 -- are at or below V.  Wants rem_ (V - the node's lower bound, from round 1)
// and the mask registers c1_..c4_ declared; leaves nb_ = the entries at or below V over the quad (the symbol's low four
// bits), lo_ = V - the largest of them, rg_ = the distance from that one to the next.
#define RCX_QUAD_ROUND2_CUM(V, Q1, Q2, Q3, Q4)                                                                         \
    u32 lo_, rg_, nb_, hi_, y1_, y2_, y3_, y4_;                                                                       \
    asm volatile("v_sub_co_u32_e64 %[y1], %[c1], %[v], %[q1]\n\t"                                                     \
                 "v_sub_co_u32_e64 %[y2], %[c2], %[v], %[q2]\n\t"                                                     \
                 "v_sub_co_u32_e64 %[y3], %[c3], %[v], %[q3]\n\t"                                                     \
                 "v_sub_co_u32_e64 %[y4], %[c4], %[v], %[q4]\n\t"                                                     \
                 "v_subb_co_u32_e64 %[nb], %[c1], 4, 0, %[c1]\n\t"                                                    \
                 "v_min3_u32 %[lo], %[y1], %[y2], %[y3]\n\t"                                                          \
                 "v_subb_co_u32_e64 %[nb], %[c2], %[nb], 0, %[c2]\n\t"                                                \
                 "v_max3_u32 %[hi], %[y1], %[y2], %[y3]\n\t"                                                          \
                 "v_subb_co_u32_e64 %[nb], %[c3], %[nb], 0, %[c3]\n\t"                                                \
                 "v_min3_u32 %[lo], %[lo], %[y4], %[rem]\n\t"                                                         \
                 "v_subb_co_u32_e64 %[nb], %[c4], %[nb], 0, %[c4]\n\t"                                                \
                 "v_max_u32 %[hi], %[hi], %[y4]\n\t"                                                                  \
                 "v_min_u32_dpp %[lo], %[lo], %[lo] " RCX_QP1                                                         \
                 "v_add_u32_dpp %[nb], %[nb], %[nb] " RCX_QP1                                                         \
                 "v_max_u32_dpp %[hi], %[hi], %[hi] " RCX_QP1                                                         \
                 "v_min_u32_dpp %[lo], %[lo], %[lo] " RCX_QP2                                                         \
                 "v_add_u32_dpp %[nb], %[nb], %[nb] " RCX_QP2                                                         \
                 "v_max_u32_dpp %[hi], %[hi], %[hi] " RCX_QP2                                                         \
                 "v_sub_u32 %[rg], %[lo], %[hi]"                                                                      \
                 : [lo] "=&v"(lo_), [rg] "=&v"(rg_), [nb] "=&v"(nb_), [hi] "=&v"(hi_), [y1] "=&v"(y1_),               \
                   [y2] "=&v"(y2_), [y3] "=&v"(y3_), [y4] "=&v"(y4_), [c1] "=&s"(c1_), [c2] "=&s"(c2_),               \
                   [c3] "=&s"(c3_), [c4] "=&s"(c4_)                                                                   \
                 : [v] "v"(V), [q1] "v"(Q1), [q2] "v"(Q2), [q3] "v"(Q3), [q4] "v"(Q4),                                \
                   [rem] "v"(rem_));;

// The 16 symbols of the fast loops: SYMBOL(HP, WORD, SHIFT) makes the byte of the symbol BEFORE it (HP = 1) into WORD at
// bit SHIFT, FINISH(WORD, SHIFT) that of the last.
#define RCX_QUAD_16_SYMBOLS(SYMBOL, FINISH)                                                                            \
    SYMBOL(0, w0_, 0) SYMBOL(1, w0_, 0) SYMBOL(1, w0_, 8) SYMBOL(1, w0_, 16)                                           \
    SYMBOL(1, w0_, 24) SYMBOL(1, w1_, 0) SYMBOL(1, w1_, 8) SYMBOL(1, w1_, 16)                                          \
    SYMBOL(1, w1_, 24) SYMBOL(1, w2_, 0) SYMBOL(1, w2_, 8) SYMBOL(1, w2_, 16)                                          \
    SYMBOL(1, w2_, 24) SYMBOL(1, w3_, 0) SYMBOL(1, w3_, 8) SYMBOL(1, w3_, 16)                                          \
    FINISH(w3_, 24)

// Symbol by symbol from index FROM (a multiple of 16: the top-ups stay 16 symbols apart), where the fast loop does not
// run; the quad's leader stores the byte.  EACH: statements for every index, decoded or not; GATHER: what makes the byte
// out of the lanes' words (nothing where every lane has it).
#define RCX_QUAD_TAIL(FROM, EACH, SYMBOL, FINISH, GATHER)                                                              \
    for (u32 i = (FROM); i < maxlen; ++i) {                                                                            \
        if ((i & 15u) == 0) in.topup();                                                                                \
        EACH                                                                                                           \
        if (i < len) { /* the 4 lanes of a quad agree */                                                               \
            u32 sym = 0;                                                                                               \
            SYMBOL(0, sym, 0);                                                                                         \
            FINISH(sym, 0);                                                                                            \
            sym = GATHER(sym);                                                                                         \
            if (leader) out[i] = (u8)sym;                                                                              \
        }                                                                                                              \
    }

// A workgroup is WAVES independent waves: with few blocks, 4 waves per workgroup land one on each SIMD of a
// CU (single-wave workgroups do not: measured 25.4 -> 19.3 ms per GiB at 16384 blocks).
#define RCX_QUAD_DEC_WAVES 4
template <int WAVES, class G = RcxBlocks>
__global__ __launch_bounds__(64 * WAVES) void rcx_dec_quad_k(const u8* __restrict__ comp, u64 comp_size, const u64* __restrict__ offsets,
                                                             u64 nblocks, u32 block, u64 n, u8* __restrict__ dst,
                                                             const u32* __restrict__ divq, u32* status,
                                                             u32* __restrict__ redo, u32 quads_used, const G g = G())
{
    __shared__ __attribute__((aligned(256))) u8 lds_all[WAVES * RCX_QUAD_LDS_BYTES];
    RCX_QUAD_SEAT(seat, WAVES, quads_used, lds_all, g, nblocks, n, block);

    // model: cpprcoder.h:1094-1132, every count 1 -- kept negated in LDS, as the bounds are in registers: round 2 below
    {
        U4 v;
        v.x = v.y = v.z = v.w = ~0u;
#pragma unroll
        for (u32 q = 0; q < 17; ++q) seat.leaves[q * 16] = v; // 16 nodes + the scratch row (which holds counts for nobody)
    }
    u32 nU1 = 0u - (64u * seat.j + 16), nU2 = nU1 - 16, nU3 = nU1 - 32, nU4 = nU1 - 48; // the bounds, negated
    const u32 T0 = 4u * seat.j;
    const u32 m1 = (seat.j & 1u) ? ~0u : 0u, m2 = (seat.j & 2u) ? ~0u : 0u;

    QuadInput in;
    u64 stream_len = 0;
    if (live) {
        RCX_STREAM(g, seat.blk, offsets);
        if (!RCX_STREAM_OK(comp_size, 9)) {
            RCX_QUAD_FAIL(seat, g, status)
        } else {
            const u32 declared = in.begin(comp + s0, comp + s1, seat.ring, seat.parked + 3);
            if (declared != len) {
                RCX_QUAD_FAIL(seat, g, status)
            }
        }
    }
    if (!live) in.idle(comp, seat.ring, seat.parked + 3);

    const u32 maxlen = rcx_wave_max(len);
    u8* out = dst + at;
    // The fast loops (a pass of 64 symbols, then 16 symbols at a go; no per-symbol length test, 16-byte stores) run as
    // far as every block of the wave has whole groups of 16 and its output is 16-byte aligned; the rest -- the ragged
    // end of a buffer's last block, the whole wave if an output is unaligned -- is decoded symbol by symbol behind them.
    // The item geometry keeps the fast loop whatever the outputs' alignment (an item begins where the one before it
    // ends): all quads stay at the same symbol index, and the 16-byte stores go to byte addresses (rcx_store16).
    u32 fast_end;
    {
        u32 mine = live ? (len & ~15u) : 0xFFFFFFF0u; // (a quad without a block sets no limit)
        if (!G::items && live && (reinterpret_cast<uintptr_t>(out) & 15u) != 0) mine = 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u32 other = (u32)__shfl_xor((int)mine, o, 64);
            mine = mine < other ? mine : other;
        }
        fast_end = mine == 0xFFFFFFF0u ? 0u : mine;
    }
    const bool leader = live && seat.in_use && seat.j == 0;

    // One symbol; the owning lane ORs it into WORD at bit SHIFT (the quad's other lanes OR in 0).
    //
    // The three arithmetic cores are written out as instruction sequences: a lone wave pays 4 cycles
    // for every s_nop the compiler has to put between a compare and the use of its mask, or between
    // a vector write and a DPP read of it (2 wait states each on gfx950), so round 2's compares go to
    // different mask registers before any is used, and every DPP step has two independent
    // instructions in front of it.  Only register-to-register vector instructions are in there;
    // LDS and global accesses stay with the compiler (and its s_waitcnt placement).
    const u32 T0p3x4 = 4u * (T0 + 3); // the lane's last symbol of a node, scaled like the symbol (below)
    const u32 leaves_lds = (u32)reinterpret_cast<uintptr_t>(seat.leaves); // low half of a flat LDS address = the LDS offset
    const u32 ring_lds = (u32)reinterpret_cast<uintptr_t>(seat.ring);
#if defined(RCX_STAMP_DEC) /* diagnostic build only (tools/diag/stamp_quad.py): where does one symbol's time go? */
#define RCX_QUAD_STAMP(i) if (stamp_now_) stamp_t_[stamp_at_ + (i)] = __builtin_amdgcn_s_memtime();
#define RCX_QUAD_NO_STAMP /* where a symbol is not timed */                                                \
    const bool stamp_now_ = false;                                                                         \
    const int stamp_at_ = 0;                                                                               \
    unsigned long long stamp_t_[4];
#else
#define RCX_QUAD_STAMP(i)
#define RCX_QUAD_NO_STAMP
#endif
// What a symbol leaves for the one behind it (below): its number scaled by 4 in two parts -- p_sb4_ = 64 x node + 4 x the
// lane's last symbol, p_hs_ = the lane's three borrows (0 or -1 each), 4 x symbol = (p_hs_ << 2) + p_sb4_, valid in the
// lane that owns it --, that lane's word (-1 there, 0 in the quad's other lanes), and the LDS address of the lane's four
// counts of the node.
    u32 p_hs_ = 0, p_sb4_ = 0, p_la_ = leaves_lds, p_own_ = 0;
// {rem, 0}, the pair round 2 adds to, lives in one fixed register pair: its high half is zeroed here, once, and the
// sequence behind the leaf read writes the low half by its name (RCX_QD_REM).
#define RCX_QD_R_LO "v116"
#define RCX_QD_R_PAIR "{v[116:117]}"
    u64 R_ = 0;
// Round 2's five pairs D, Y_a, Y_b, Y_c, Y_e: fixed registers as well, written and read inside one sequence and listed as
// clobbered by it, so that the sequence can name their halves.
#define RCX_QD_D "v[118:119]"
#define RCX_QD_D_L "v118"
#define RCX_QD_D_H "v119"
#define RCX_QD_YA "v[120:121]"
#define RCX_QD_YA_L "v120"
#define RCX_QD_YA_H "v121"
#define RCX_QD_YB "v[122:123]"
#define RCX_QD_YB_L "v122"
#define RCX_QD_YB_H "v123"
#define RCX_QD_YC "v[124:125]"
#define RCX_QD_YC_L "v124"
#define RCX_QD_YC_H "v125"
#define RCX_QD_YE "v[126:127]"
#define RCX_QD_YE_L "v126"
#define RCX_QD_YE_H "v127"
#define RCX_QD_PAIRS_CLOBBERED "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127"
// One symbol.  Its byte and the +1 on its count are NOT made here but by the next symbol (HP = 1: PWORD, PSHIFT are that
// earlier symbol's word and bit position) or by RCX_QUAD_DEC_FINISH: nothing the coder state needs depends on them, so
// they fill the slots the node index's steps across the quad need anyway (the ds_add still comes before the next leaf
// read: LDS serves a wave's operations in order) and the wait for the leaf read.
// The counts are kept negated (a symbol seen c times: -c), so the +1 is a ds_add of the owner word as it is, and the byte
// is the symbol ANDed with it; the first byte of an output word (PSHIFT == 0) IS the word.
// The symbol is carried scaled by 4 (psym4), because its count's address is then ONE bit insert: bits 2 and 3 of psym4
// into the 16-byte aligned address of the lane's four counts.  The bit insert is also what bounds the address: whatever
// psym4 holds -- in a block that took "node 16" the borrows are arbitrary words -- the result lies in [pla, pla + 12],
// inside the lane's own 16 bytes of the row round 1 chose (an add of 4 x the borrows to pla would not: the ds_add of a
// damaged block would land in another wave's tables).  psym4 & pown is 4 x the byte: it goes into the word at PSHIFT - 2,
// and the first byte of a word is shifted down.
#define RCX_QD_PREV_A_0 "s_nop 1\n\t"
#define RCX_QD_PREV_A_1 "v_lshl_add_u32 %[psym4], %[phs], 2, %[psb4]\n\t"                                           \
                        "v_bfi_b32 %[pad], 12, %[psym4], %[pla]\n\t" /* LDS address of the earlier symbol's count */
#define RCX_QD_PREV_S_FIRST "v_and_b32 %[pword], %[psym4], %[pown]\n\t"                                             \
                            "v_lshrrev_b32 %[pword], 2, %[pword]\n\t"
#define RCX_QD_PREV_S_NEXT "v_and_b32 %[pye], %[psym4], %[pown]\n\t"                                                \
                           "v_lshl_or_b32 %[pword], %[pye], %[psh], %[pword]\n\t"
#define RCX_QP3 "quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
/* behind the leaf read: the remainder (round 1's other result) across the quad, and as the pair {rem, 0} round 2 adds to; \
   cpprcoder.h:1134-1177, +1 on every cumulative sum above the node -- the bounds whose subtraction borrowed in round 1  \
   (bound above low <=> its node number above the symbol's node; a target past the total leaves no borrow and raises    \
   none, as find()'s fall-through needs it): the negated bound takes its high word, 0 or -1; the earlier symbol's byte */ \
#define RCX_QD_REM(PREV, PSHIFT, ...)                                                                      \
        asm volatile("v_min3_u32 %[rm], %[x1], %[x2], %[x3]\n\t"                                           \
                     "v_min3_u32 %[rm], %[rm], %[x4], %[low]\n\t"                                          \
                     "v_add_u32 %[u1], %[u1], %[h1]\n\t"                                                   \
                     "v_add_u32 %[u2], %[u2], %[h2]\n\t"                                                   \
                     "v_min_u32_dpp %[rm], %[rm], %[rm] " RCX_QP1                                          \
                     "v_add_u32 %[u3], %[u3], %[h3]\n\t"                                                   \
                     "v_add_u32 %[u4], %[u4], %[h4]\n\t"                                                   \
                     "v_min_u32_dpp " RCX_QD_R_LO ", %[rm], %[rm] " RCX_QP2 /* the low half of R; its high half stays 0 */ \
                     PREV                                                                                  \
                     : [u1] "+v"(nU1), [u2] "+v"(nU2), [u3] "+v"(nU3), [u4] "+v"(nU4), [rm] "=&v"(rem_),    \
                       [R] "+" RCX_QD_R_PAIR(R_) __VA_ARGS__                                                \
                     : [low] "v"(in.low), [x1] "v"(x1_), [x2] "v"(x2_),                                    \
                       [x3] "v"(x3_), [x4] "v"(x4_), [h1] "v"(h1_), [h2] "v"(h2_), [h3] "v"(h3_), [h4] "v"(h4_), \
                       [pown] "v"(p_own_), [psym4] "v"(psym4_), [psh] "n"((PSHIFT) > 2 ? (PSHIFT)-2 : 0))
#define RCX_QUAD_DEC_SYMBOL(MUL, INC, SH, HP, PWORD, PSHIFT)                                               \
    {                                                                                                      \
        /* cpprcoder.h:926-940 (in.n4 = the next four stream bytes, ready since the previous symbol) */    \
        const u32 k8_ = rcx_clz(in.range) & 0x18u;                                                         \
        in.low = (u32)((((u64)in.low << 32) | in.n4) << k8_ >> 32);                                        \
        /* :904, range / total by the table entry (RCX_QUAD_DIVQ_DW); the renormalised range is below 2^32 - 255 (a     \
           range is count x t <= (total - 255) x t, or shifted left by 8 or more), so range + inc does not wrap (only a block \
           that has already decoded "node 16" can break that, and it is marked and decoded again) */          \
        const u32 t_ = __umulhi((in.range << k8_) + (INC), (MUL)) >> (SH);                                 \
        /* round 1: which of the 16 nodes.  node = bounds at or below low, rem = low - the largest.  One 64-bit           \
           multiply-add per bound: {low, 0} - U_k * t has low - U_k * t in its low word and the borrow, 0 or -1, in   \
           its high word (its carry-out goes to a mask register nothing reads) */                          \
        const u64 lowp_ = in.low;                                                                          \
        u32 node_, rem_, ro_, la_, pad_, pye_, psym4_;                                                     \
        u64 X1_, X2_, X3_, X4_, cz_, cy_;                                                                  \
        asm volatile("v_mad_i64_i32 %[X1], %[cz], %[n1], %[t], %[lp]\n\t"                                  \
                     "v_mad_i64_i32 %[X2], %[cz], %[n2], %[t], %[lp]\n\t"                                  \
                     "v_mad_i64_i32 %[X3], %[cz], %[n3], %[t], %[lp]\n\t"                                  \
                     "v_mad_i64_i32 %[X4], %[cz], %[n4], %[t], %[lp]"                                      \
                     : [X1] "=&v"(X1_), [X2] "=&v"(X2_), [X3] "=&v"(X3_), [X4] "=&v"(X4_), [cz] "=&s"(cz_)  \
                     : [n1] "v"(nU1), [n2] "v"(nU2), [n3] "v"(nU3), [n4] "v"(nU4), [t] "v"(t_), [lp] "v"(lowp_)); \
        /* (a statement that reads the words of the pairs cannot come right behind the one that wrote them without an   \
           s_nop from the compiler: the stream position moves on in between) */                            \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        in.bp8 += k8_;                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        const u32 x1_ = (u32)X1_, x2_ = (u32)X2_, x3_ = (u32)X3_, x4_ = (u32)X4_;                          \
        const u32 h1_ = (u32)(X1_ >> 32), h2_ = (u32)(X2_ >> 32), h3_ = (u32)(X3_ >> 32), h4_ = (u32)(X4_ >> 32); \
        asm volatile("v_add3_u32 %[nd], %[h1], %[h2], %[h3]\n\t"                                           \
                     "v_add3_u32 %[nd], %[nd], %[h4], 4\n\t" /* 4 - the lane's borrows (they stay: the update below) */ \
                     RCX_QD_PREV_A_##HP                                                                    \
                     : [nd] "=&v"(node_), [pad] "=&v"(pad_), [psym4] "=&v"(psym4_)                          \
                     : [h1] "v"(h1_), [h2] "v"(h2_), [h3] "v"(h3_), [h4] "v"(h4_),                         \
                       [phs] "v"(p_hs_), [psb4] "v"(p_sb4_), [pla] "v"(p_la_));                            \
        if (HP) (void)__hip_atomic_fetch_add(reinterpret_cast<RcxLdsU32*>(pad_), p_own_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); /* :916, the earlier symbol's: -1 on its negated count */ \
        asm volatile("v_add_u32_dpp %[nd], %[nd], %[nd] " RCX_QP1                                          \
                     "v_bfe_u32 %[ro], %[bp], 5, 5\n\t"  /* ring slot of the next pair ... */               \
                     "v_lshl_add_u32 %[ro], %[ro], 2, %[rb]" /* ... and its LDS address (formed here: a vector instruction right \
                                                               behind the sequence that reads a register of it costs an s_nop) */ \
                     : [nd] "+v"(node_), [ro] "=&v"(ro_)                                                    \
                     : [bp] "v"(in.bp8), [rb] "v"(ring_lds));                                              \
        {                                                                                                  \
            const RcxLdsU32* at_ = reinterpret_cast<const RcxLdsU32*>(ro_); /* the stream bytes of the next symbol */ \
            in.w0 = at_[0];                                                                                \
            in.w1 = at_[1];                                                                                \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        asm volatile("v_add_u32_dpp %[nd], %[nd], %[nd] " RCX_QP2                                          \
                     "v_lshl_add_u32 %[la], %[nd], 8, %[lvb]" /* LDS address of the lane's 4 counts of the node */ \
                     : [nd] "+v"(node_), [la] "=&v"(la_)                                                    \
                     : [lvb] "v"(leaves_lds));                                                             \
        /* round 2: which of the node's 16 symbols */                                                      \
        RCX_QUAD_STAMP(0);                                                                                 \
        const RcxV4 l_ = *reinterpret_cast<const RcxLdsV4*>(la_);                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (!(HP)) RCX_QD_REM("", 0);                                                                      \
        else if ((PSHIFT) == 0) RCX_QD_REM(RCX_QD_PREV_S_FIRST, 0, , [pword] "=&v"(PWORD));                \
        else RCX_QD_REM(RCX_QD_PREV_S_NEXT, PSHIFT, , [pye] "=&v"(pye_), [pword] "+v"(PWORD));             \
        /* The lane's four counts l are negative.  P = the counts of the node's symbols in lower lanes (negated, from the \
           lanes' unscaled sums across the quad), D = {rem, 0} + P x t, and Y_k = Y_(k-1) + l_k x t from Y_0 = D: the low \
           words are rem - t x (the counts up to and including the lane's k-th), the high words their borrows.  In the \
           lane that owns the symbol and below it D >= 0 and every high word is 0 or -1; above it D < 0, -1 or -2. */ \
        /* The five pairs are fixed registers (RCX_QD_D ... RCX_QD_YE, scratch of this one sequence): their words have   \
           names, so nothing of the compiler's has to stand between the multiply-adds and what reads their halves. */ \
        u32 qe_, pre_, o2_, o3_;                                                                           \
        u32 lo_, rg_, hi_;                                                                                 \
        asm volatile("v_add3_u32 %[qe], %[lx], %[ly], %[lz]\n\t"                                           \
                     "v_add_u32 %[qe], %[qe], %[lw]\n\t"                                                   \
                     "v_alignbit_b32 %[n4], %[w1], %[w0], %[bp]\n\t" /* (the next symbol's 4 stream bytes at bp8 ... */ \
                     "v_perm_b32 %[n4], %[n4], %[n4], %[swap]\n\t" /* ... first one on top: here they separate qe from its use across the quad) */ \
                     "v_and_b32_dpp %[pre], %[qe], %[m1] " RCX_QP1 /* all three steps read the lane's own sum: no wait between them */ \
                     "v_and_b32_dpp %[o2], %[qe], %[m2] " RCX_QP2                                          \
                     "v_and_b32_dpp %[o3], %[qe], %[m2] " RCX_QP3                                          \
                     "v_add3_u32 %[qe], %[pre], %[o2], %[o3]\n\t" /* P */                                        \
                     "v_mad_i64_i32 " RCX_QD_D ", %[cy], %[qe], %[t], %[R]\n\t"                             \
                     "v_mad_i64_i32 " RCX_QD_YA ", %[cy], %[lx], %[t], " RCX_QD_D "\n\t"                    \
                     "v_mad_i64_i32 " RCX_QD_YB ", %[cy], %[ly], %[t], " RCX_QD_YA "\n\t"                   \
                     "v_mad_i64_i32 " RCX_QD_YC ", %[cy], %[lz], %[t], " RCX_QD_YB "\n\t"                   \
                     "v_mad_i64_i32 " RCX_QD_YE ", %[cy], %[lw], %[t], " RCX_QD_YC "\n\t"                   \
                     "v_min3_u32 %[lo], " RCX_QD_D_L ", " RCX_QD_YA_L ", " RCX_QD_YB_L "\n\t"              \
                     "v_max3_u32 %[hi], " RCX_QD_YA_L ", " RCX_QD_YB_L ", " RCX_QD_YC_L "\n\t"             \
                     "v_min_u32 %[lo], %[lo], " RCX_QD_YC_L "\n\t"                                         \
                     "v_max_u32 %[hi], %[hi], " RCX_QD_YE_L "\n\t"                                         \
                     "v_add3_u32 %[hs], " RCX_QD_YA_H ", " RCX_QD_YB_H ", " RCX_QD_YC_H "\n\t" /* the symbol = the lane's last one + these three borrows */ \
                     "v_min_u32_dpp %[lo], %[lo], %[lo] " RCX_QP1                                          \
                     "v_max_u32_dpp %[hi], %[hi], %[hi] " RCX_QP1                                          \
                     "v_bfi_b32 %[own], " RCX_QD_D_H ", 0, " RCX_QD_YE_H "\n\t" /* ~h_D & h_e: -1 in the lane that owns the symbol, 0 elsewhere */ \
                     "v_min_u32_dpp %[lo], %[lo], %[lo] " RCX_QP2                                          \
                     "v_max_u32_dpp %[hi], %[hi], %[hi] " RCX_QP2                                          \
                     "v_sub_u32 %[rg], %[lo], %[hi]"                                                       \
                     : [n4] "=&v"(in.n4), [qe] "=&v"(qe_), [pre] "=&v"(pre_), [o2] "=&v"(o2_), [o3] "=&v"(o3_), \
                       [lo] "=&v"(lo_), [rg] "=&v"(rg_), [hs] "=&v"(p_hs_), [own] "=&v"(p_own_), [hi] "=&v"(hi_), \
                       [cy] "=&s"(cy_)                                                                      \
                     : [lx] "v"(l_.x), [ly] "v"(l_.y), [lz] "v"(l_.z), [lw] "v"(l_.w), [t] "v"(t_),        \
                       [R] "v"(R_), [m1] "v"(m1), [m2] "v"(m2),                                            \
                       [w0] "v"(in.w0), [w1] "v"(in.w1), [bp] "v"(in.bp8), [swap] "s"(0x00010203u)         \
                     : RCX_QD_PAIRS_CLOBBERED);                                                            \
        /* The compiler's first vector instruction behind a sequence costs an s_nop 0 if it touches a register the      \
           sequence wrote.  So the one that stands there reads none of them: 4 x (16 x node + the lane's last symbol),    \
           the part of the scaled symbol that round 1 decided, which the next symbol adds the borrows to.  Nor may it    \
           write one: the empty statement behind it keeps the sequence's scratch registers taken and the pairs' out of  \
           its reach (round 7's remedy; it leans on nothing but the operands). */                          \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        p_sb4_ = (node_ << 6) + T0p3x4;                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        asm volatile("" : : "v"(p_sb4_), "v"(qe_), "v"(pre_), "v"(o2_), "v"(o3_), "v"(hi_) : RCX_QD_PAIRS_CLOBBERED); \
        RCX_QUAD_STAMP(1);                                                                                 \
        in.low = lo_;   /* :906 */                                                                         \
        in.range = rg_; /* :907 */                                                                         \
        p_la_ = la_;                                                                                       \
    }
// The byte and the count of the last symbol decoded (no symbol follows that would make them): into WORD at bit SHIFT.
#define RCX_QD_FINISH(BYTE, SHIFT, ...)                                                                    \
        asm volatile(RCX_QD_PREV_A_1                                                                       \
                     BYTE                                                                                  \
                     : [pad] "=&v"(pad_), [psym4] "=&v"(psym4_) __VA_ARGS__                                 \
                     : [pown] "v"(p_own_), [phs] "v"(p_hs_), [psb4] "v"(p_sb4_), [pla] "v"(p_la_),         \
                       [psh] "n"((SHIFT) > 2 ? (SHIFT)-2 : 0))
#define RCX_QUAD_DEC_FINISH(WORD, SHIFT)                                                                    \
    {                                                                                                      \
        u32 pad_, pye_, psym4_;                                                                            \
        if ((SHIFT) == 0) RCX_QD_FINISH(RCX_QD_PREV_S_FIRST, 0, , [pword] "=&v"(WORD));                    \
        else RCX_QD_FINISH(RCX_QD_PREV_S_NEXT, SHIFT, , [pye] "=&v"(pye_), [pword] "+v"(WORD));            \
        (void)__hip_atomic_fetch_add(reinterpret_cast<RcxLdsU32*>(pad_), p_own_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); /* :916 */ \
    }

    // The divisors of the fast loop: a quarter group -- multipliers and increments of 4 symbols -- sits in two 16-byte
    // registers that every lane loads alike, and is loaded again, with the next group's quarter, right behind the
    // quarter's last symbol: 13 symbols ahead of the first use, and no register copies between groups.  These are vector
    // loads (vmcnt), which the loop waits for only at the top-up; a scalar load would share lgkmcnt with LDS and, as it
    // returns out of order, make the next symbol's leaf-read wait a wait for it as well (RCX_QUAD_DIV_SMEM: that variant).
#if defined(RCX_QUAD_DIV_SMEM)
    const u32* dq_ = divq; // a uniform address: scalar loads
#else
    u32 vz_;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz_)); // a zero the compiler cannot see through: the loads stay vector loads
    const u32* dq_ = divq + vz_;
#endif
#define RCX_QUAD_DIVQ_LOAD(G, Q)                                                                             \
    {                                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        dm##Q = reinterpret_cast<const U4*>(dq_ + (G) * RCX_QUAD_DIVQ_DW)[Q];                              \
        di##Q = reinterpret_cast<const U4*>(dq_ + (G) * RCX_QUAD_DIVQ_DW + 16)[Q];                         \
    }
#define RCX_QUAD_U4_AT(V, C) ((C) == 0 ? (V).x : (C) == 1 ? (V).y : (C) == 2 ? (V).z : (V).w)
    {
        U4 o_last;
        o_last.x = o_last.y = o_last.z = o_last.w = 0;
#if defined(RCX_STAMP_DEC)
        unsigned long long stamp_sum_[4] = {0, 0, 0, 0};
#endif
        U4 dm0, dm1, dm2, dm3, di0, di1, di2, di3;
        RCX_QUAD_DIVQ_LOAD(0u, 0) RCX_QUAD_DIVQ_LOAD(0u, 1) RCX_QUAD_DIVQ_LOAD(0u, 2) RCX_QUAD_DIVQ_LOAD(0u, 3)
        // These eight are waited for here, once, by a statement that reads them.  Left pending into the loops, the order the
        // compiler gave them (the first quarter last) decides what the loop's first vmcnt wait allows for every pass, not
        // only the first: vmcnt(1), which waits for the stores in front of it and for the piece just requested.
        asm volatile("" ::"v"(dm0.x), "v"(di0.x), "v"(dm1.x), "v"(di1.x), "v"(dm2.x), "v"(di2.x), "v"(dm3.x), "v"(di3.x));
#if defined(RCX_STAMP_DEC)
#define RCX_QUAD_STEP(S, Q, HP, PW)                                                                           \
    {                                                                                                        \
        const bool stamp_now_ = (S) == 8 || (S) == 9;                                                        \
        const int stamp_at_ = (S) == 8 ? 0 : 2;                                                              \
        RCX_QUAD_DEC_SYMBOL(RCX_QUAD_U4_AT(dm##Q, (S) & 3), RCX_QUAD_U4_AT(di##Q, (S) & 3), sh_, HP, PW,     \
                            (8 * (((S) + 3) & 3)));                                                          \
    }
#else
#define RCX_QUAD_STEP(S, Q, HP, PW)                                                                           \
    RCX_QUAD_DEC_SYMBOL(RCX_QUAD_U4_AT(dm##Q, (S) & 3), RCX_QUAD_U4_AT(di##Q, (S) & 3), sh_, HP, PW, (8 * (((S) + 3) & 3)));
#endif
// A group: 16 symbols with the shift sh_, the divisors of group GN loaded behind each quarter, the quad's 16 bytes into O
// (a step makes the byte of the step before it: RCX_QUAD_DEC_SYMBOL)
#define RCX_QUAD_GROUP(GN, O)                                                                                 \
    {                                                                                                        \
        u32 w0_ = 0, w1_ = 0, w2_ = 0, w3_ = 0;                                                              \
        RCX_QUAD_STEP(0, 0, 0, w0_) RCX_QUAD_STEP(1, 0, 1, w0_) RCX_QUAD_STEP(2, 0, 1, w0_) RCX_QUAD_STEP(3, 0, 1, w0_) \
        RCX_QUAD_DIVQ_LOAD(GN, 0)                                                                            \
        RCX_QUAD_STEP(4, 1, 1, w0_) RCX_QUAD_STEP(5, 1, 1, w1_) RCX_QUAD_STEP(6, 1, 1, w1_) RCX_QUAD_STEP(7, 1, 1, w1_) \
        RCX_QUAD_DIVQ_LOAD(GN, 1)                                                                            \
        RCX_QUAD_STEP(8, 2, 1, w1_) RCX_QUAD_STEP(9, 2, 1, w2_) RCX_QUAD_STEP(10, 2, 1, w2_) RCX_QUAD_STEP(11, 2, 1, w2_) \
        RCX_QUAD_DIVQ_LOAD(GN, 2)                                                                            \
        RCX_QUAD_STEP(12, 3, 1, w2_) RCX_QUAD_STEP(13, 3, 1, w3_) RCX_QUAD_STEP(14, 3, 1, w3_) RCX_QUAD_STEP(15, 3, 1, w3_) \
        RCX_QUAD_DIVQ_LOAD(GN, 3)                                                                            \
        RCX_QUAD_DEC_FINISH(w3_, 24)                                                                         \
        (O).x = rcx_quad_or(w0_);                                                                            \
        (O).y = rcx_quad_or(w1_);                                                                            \
        (O).z = rcx_quad_or(w2_);                                                                            \
        (O).w = rcx_quad_or(w3_);                                                                            \
    }
        u32 i0 = 0;
#if !defined(RCX_STAMP_DEC) /* (the diagnostic build times symbols of the loop of 16 below, so there that loop runs alone) */
        // The pass: 64 symbols, four groups with their top-ups, while every block of the wave has them.  Which of the four
        // a group is, is known when the kernel is compiled, so the 64 bytes wait in registers -- the scratch row takes none
        // of them --, they leave as four stores behind the NEXT pass's first top-up (the rule above), and the shift (the
        // powers of two from 256 up are multiples of 64), the test for the stores and the loop's own instructions are
        // issued once per 64 symbols where the loop of 16 issues them four times.
        {
            U4 o_p0 = o_last, o_p1 = o_last, o_p2 = o_last;
            for (; i0 + 64 <= fast_end; i0 += 64) {
                in.topup();
                if (i0 != 0 && leader) {
                    u8* o4 = out + (i0 - 64);
                    rcx_store16<G::items>(o4, o_p0);
                    rcx_store16<G::items>(o4 + 16, o_p1);
                    rcx_store16<G::items>(o4 + 32, o_p2);
                    rcx_store16<G::items>(o4 + 48, o_last);
                }
                const u32 sh_ = 31u - (u32)__builtin_clz(256u + i0); // floor(log2(total)), the same for the four groups
                const u32 gn_ = (i0 >> 4) + 1u;
                RCX_QUAD_GROUP(gn_, o_p0)
                in.topup();
                RCX_QUAD_GROUP(gn_ + 1u, o_p1)
                in.topup();
                RCX_QUAD_GROUP(gn_ + 2u, o_p2)
                in.topup();
                RCX_QUAD_GROUP(gn_ + 3u, o_last)
            }
            // The last pass's 64 bytes go where the loop of 16 keeps its own: it starts at a multiple of 64 and sends them
            // off behind its first top-up, or RCX_QUAD_PARKED_END does.
            if (i0 != 0) seat.parked[0] = o_p0, seat.parked[1] = o_p1, seat.parked[2] = o_p2;
        }
#endif
        // The whole groups that are left (fewer than four behind the pass), their output parked as the macros above say.
        for (; i0 < fast_end; i0 += 16) {
            in.topup();
            RCX_QUAD_PARKED_FLUSH(i0, seat.parked, o_last, G::items)
            const u32 sh_ = 31u - (u32)__builtin_clz(256u + i0); // floor(log2(total)), the group's shift
            const u32 gn_ = (i0 >> 4) + 1u;                      // the next group
#if defined(RCX_STAMP_DEC)
            unsigned long long stamp_t_[4] = {0, 0, 0, 0};
#endif
            U4 o;
            RCX_QUAD_GROUP(gn_, o)
#if defined(RCX_STAMP_DEC)
            stamp_sum_[0] += stamp_t_[1] - stamp_t_[0]; // symbol 8: leaf read issued -> round 2 done
            stamp_sum_[1] += stamp_t_[2] - stamp_t_[1]; // -> leaf read of symbol 9 issued
            stamp_sum_[2] += stamp_t_[3] - stamp_t_[2]; // symbol 9: leaf read issued -> round 2 done
            stamp_sum_[3] += 1;
#endif
            RCX_QUAD_PARKED_PUT(o, seat.parked, o_last);
        }
#undef RCX_QUAD_GROUP
#undef RCX_QUAD_STEP
#if defined(RCX_STAMP_DEC)
        if (blockIdx.x == 7 && threadIdx.x == 0)
            for (int i_ = 0; i_ < 4; ++i_) rcx_dec_stamp_out[i_] = stamp_sum_[i_];
#endif
        RCX_QUAD_PARKED_END(fast_end, seat.parked, o_last, G::items)
    }
    {
        u32 mul_n_, inc_n_;
#define RCX_QUAD_DIVQ_ENTRY(I)                                                                              \
    {                                                                                                      \
        const u32* e_ = divq + ((I) >> 4) * RCX_QUAD_DIVQ_DW + ((I) & 15u);                                 \
        mul_n_ = e_[0];                                                                                    \
        inc_n_ = e_[16];                                                                                   \
    }
        RCX_QUAD_DIVQ_ENTRY(fast_end);
        // one symbol ahead (entry maxlen exists: the table covers the block and more)
#define RCX_QUAD_TAIL_EACH                                                                                  \
    const u32 mul_ = mul_n_, inc_ = inc_n_, sh_ = 31u - (u32)__builtin_clz(256u + i);                      \
    RCX_QUAD_DIVQ_ENTRY(i + 1u);                                                                           \
    RCX_QUAD_NO_STAMP
#define RCX_QUAD_TAIL_SYMBOL(HP, WORD, SHIFT) RCX_QUAD_DEC_SYMBOL(mul_, inc_, sh_, HP, WORD, SHIFT)
        RCX_QUAD_TAIL(fast_end, RCX_QUAD_TAIL_EACH, RCX_QUAD_TAIL_SYMBOL, RCX_QUAD_DEC_FINISH, rcx_quad_or)
#undef RCX_QUAD_TAIL_EACH
#undef RCX_QUAD_TAIL_SYMBOL
    }
#undef RCX_QUAD_DEC_SYMBOL
#undef RCX_QUAD_DEC_FINISH
#undef RCX_QD_PREV_A_0
#undef RCX_QD_PREV_A_1
#undef RCX_QD_PREV_S_FIRST
#undef RCX_QD_PREV_S_NEXT
#undef RCX_QD_REM
#undef RCX_QD_FINISH
#undef RCX_QD_R_LO
#undef RCX_QD_R_PAIR
#undef RCX_QD_D
#undef RCX_QD_D_L
#undef RCX_QD_D_H
#undef RCX_QD_YA
#undef RCX_QD_YA_L
#undef RCX_QD_YA_H
#undef RCX_QD_YB
#undef RCX_QD_YB_L
#undef RCX_QD_YB_H
#undef RCX_QD_YC
#undef RCX_QD_YC_L
#undef RCX_QD_YC_H
#undef RCX_QD_YE
#undef RCX_QD_YE_L
#undef RCX_QD_YE_H
#undef RCX_QD_PAIRS_CLOBBERED
#undef RCX_QP3
#undef RCX_QUAD_DIVQ_LOAD
#undef RCX_QUAD_DIVQ_ENTRY
#undef RCX_QUAD_U4_AT
    // A symbol past the table ("node 16") is the only one that raises none of the cumulative sums: the last
    // lane's U4 -- the total, 256 + the symbols decoded (cpprcoder.h:1096, :1138) -- then falls short.
    // A marked block is judged (truncated or not) by the kernel that decodes it again.
    const bool marked = live && rcx_quad_or(seat.j == 3 && 0u - nU4 != 256u + len ? 1u : 0u) != 0;
    if (leader && !marked && in.taken() > stream_len) rcx_flag(status, RCX_ST_CORRUPT, rcx_id(g, seat.blk));
    RCX_QUAD_MARK_REDO(seat, redo, nblocks, marked);
}
