// rcx_static.hpp -- the static (two-pass) range coder RangeEncoder<T> on gfx950: one lane per block
// (rcx_enc_static_k, rcx_dec_static_k), and the many-wave / four-lane kernels built on rcx_mc.hpp's and rcx_quad.hpp's machinery
// (rcx_enc_static3_k, rcx_dec_static_quad_k).
//
// Reference: cpprcoder.h:321-619.  Stream of one block:
//   [u32 LE n][256 x u16 LE counts][0x00 lead-in][payload ...][u32 BE low]      (516-byte header, :331)
// encode (:375-458): count() histogram with the order-dependent 16-bit squeeze (:543-571), write16
// (:604-619), calcCumulatives (:573-583), then the same divide / multiply / carry / renormalise loop
// as the adaptive coder with a FIXED table, range starting at 0xFFFFFFFF (:382) and the tail rule
// "low == 0xFFFFFFFF bumps the held byte and fills with 0x00" (:439-451).
// decode (:460-519): table from the header, low from bytes 1..4 after it (:494-498), per symbol
// t = range/total, find(low/t) (:521-535), then renormalise.
//
// The table of a block is 257 dwords in LDS, dword-interleaved over the 64 lanes of the wave
// (entry i of lane l at (i*64 + l)*4), so any per-lane index is bank-conflict free.  The divisor
// (total) is fixed per block but differs between lanes: its multiply-add magic is computed once per
// block on the device.  Included by rcx_kernels.hpp.
#pragma once

#define RCX_STATIC_HEADER 516u
#define RCX_STATIC_LDS_DW (257 * RCX_LANES)

// (StaticTable, the table of one lane, is in rcx_lane.hpp with the one-lane decoder's symbol step: the host lane simulator
// of the tests compiles both.)

// count() (cpprcoder.h:543-571) for the symbols [from, to) of every lane's block, with the order-dependent 16-bit
// squeeze (:549-555): when a count is 0xFFFF or more BEFORE its increment, every non-zero count becomes
// (c >> 1) | 1 first.  PIECES: the blocks are whole and 16-byte aligned and `from` is a multiple of 16, so the input
// is taken 16 bytes at a time: the 16 increments are issued as returning LDS atomics, and only if one of them
// found 0xFFFF or more (a block dominated by one symbol) are they taken back and redone one by one.
__device__ __forceinline__ void rcx_static_squeeze(const StaticTable& tab)
{
    for (u32 q = 0; q < 256; ++q) {
        const u32 c = tab.get(q);
        if (c > 0) tab.set(q, (c >> 1) | 1u);
    }
}
__device__ __forceinline__ void rcx_static_count_one(const StaticTable& tab, u32 b)
{
    if (tab.get(b) >= 0xFFFFu) rcx_static_squeeze(tab);
    tab.set(b, tab.get(b) + 1);
}
template <bool PIECES>
__device__ __forceinline__ void rcx_static_count_checked(const StaticTable& tab, const u8* in, u32 from, u32 to, u32 len)
{
    u32 i = from;
    if (PIECES) {
        for (; i + 16 <= to; i += 16) {
            const U4 piece = *reinterpret_cast<const U4*>(in + i);
            u32 worst = 0;
#pragma unroll
            for (u32 s = 0; s < 16; ++s) {
                const u32 old = __hip_atomic_fetch_add(tab.col + rcx_byte_of(piece, s) * RCX_LANES, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                worst = worst > old ? worst : old;
            }
            if (rcx_any(worst >= 0xFFFFu)) {
                if (worst >= 0xFFFFu) {
                    for (u32 s = 0; s < 16; ++s) tab.set(rcx_byte_of(piece, s), tab.get(rcx_byte_of(piece, s)) - 1);
                    for (u32 s = 0; s < 16; ++s) rcx_static_count_one(tab, rcx_byte_of(piece, s));
                }
            }
        }
    }
    for (; i < to; ++i)
        if (i < len) rcx_static_count_one(tab, in[i]);
}
// The largest count of the lane's table: no squeeze can fire while it stays below 0xFFFF.
__device__ __forceinline__ u32 rcx_static_max_count(const StaticTable& tab)
{
    u32 m = 0;
    for (u32 q = 0; q < 256; ++q) {
        const u32 c = tab.get(q);
        m = m > c ? m : c;
    }
    return m;
}

// ===========================================================================
// Static encode, pass 1 (scan + scatter are shared with the adaptive coder)
// ===========================================================================
template <class G = RcxBlocks>
__global__ __launch_bounds__(64) void rcx_enc_static_k(const u8* __restrict__ src, u64 n, u32 block, u64 nblocks,
                                                       u8* __restrict__ slots, u64 slot, u32* __restrict__ sizes, u32* status,
                                                       const u32* __restrict__ only, const G g = G())
{
    __shared__ u32 lds[RCX_STATIC_LDS_DW];
    const u32 lane = threadIdx.x;
    const u64 blk = (u64)blockIdx.x * RCX_LANES + lane;
    // second pass behind rcx_enc_static3_k: only the blocks it marked (none, on ordinary data)
    RCX_ENTRY_ONLY(g, blk, nblocks, n, block, only);
    RCX_ENTRY_SLOTS(g, blk, slots, slot);
    const u8* in = src + at;
    StaticTable tab{lds + lane};

    // ---- count(), cpprcoder.h:543-571 ----
    for (u32 i = 0; i <= 256; ++i) tab.set(i, 0);
    const u32 maxlen = rcx_wave_max(len);
    const bool full = RCX_ALL_FULL(g, block, src);
    // A count can only be 0xFFFF before its increment once 65535 earlier symbols exist, so the squeeze
    // test is not needed for the first 65535 symbols of a block.
    const u32 easy = maxlen < 65535u ? maxlen : 65535u;
    if (full) {
        const u32 easy16 = easy & ~15u;
        for (u32 i = 0; i < easy16; i += 16) {
            const U4 piece = *reinterpret_cast<const U4*>(in + i);
#pragma unroll
            for (u32 s = 0; s < 16; ++s) tab.inc(rcx_byte_of(piece, s));
        }
        for (u32 i = easy16; i < easy; ++i) tab.inc(in[i]);
    } else {
        for (u32 i = 0; i < easy; ++i)
            if (i < len) tab.inc(in[i]);
    }
    if (full) {
        const u32 from = (easy + 15u) & ~15u;
        rcx_static_count_checked<false>(tab, in, easy, from < maxlen ? from : maxlen, len);
        if (from < maxlen) rcx_static_count_checked<true>(tab, in, from, maxlen, len);
    } else {
        rcx_static_count_checked<false>(tab, in, easy, maxlen, len);
    }
    // The second rescale of count() (cpprcoder.h:561-570): more than 2^24 symbols (single streams only: blocks are
    // at most RCX_MAX_BLOCK).  Entry 0 is skipped, as the reference's loop starting at 1 does.
    if (len > (1u << 24)) {
        u32 sz = len, shift = 0;
        while (sz > (1u << 24)) {
            sz >>= 1;
            ++shift;
        }
        for (u32 q = 1; q < 256; ++q) {
            const u32 c = tab.get(q);
            tab.set(q, c != 0 ? ((c >> shift) | 1u) : 0u);
        }
    }

    // ---- header: u32 LE n + 256 u16 counts (cpprcoder.h:386-397, :604-619), then the cumulative table ----
    u8* wave_slots = slots + (u64)blockIdx.x * RCX_LANES * slot;
    EncLane enc;
    if (live) {
        enc.begin(wave_slots, lane * (u32)slot, (u32)slot, len);
        u32* hdr = reinterpret_cast<u32*>(wave_slots + lane * (u32)slot + 4);
        for (u32 i = 0; i < 256; i += 2) hdr[i >> 1] = (tab.get(i) & 0xFFFFu) | (tab.get(i + 1) << 16);
        enc.off += RCX_STATIC_HEADER - 4;
        enc.cap -= RCX_STATIC_HEADER - 4;
    } else {
        enc.idle(wave_slots);
    }
    enc.range = 0xFFFFFFFFu; // cpprcoder.h:382
    const u32 total = tab.accumulate();
    const DivEntry k = rcx_make_div_entry(total ? total : 1u);

    // ---- the coding loop, cpprcoder.h:400-436 ----
    if (full) {
        U4 cur = *reinterpret_cast<const U4*>(in);
        for (u32 i = 0; i < maxlen; i += 16) {
            U4 nxt = cur;
            if (i + 16 < maxlen) nxt = *reinterpret_cast<const U4*>(in + i + 16);
#pragma unroll
            for (u32 s = 0; s < 16; ++s) {
                const u32 b = rcx_byte_of(cur, s);
                const u32 lo = tab.get(b), hi = tab.get(b + 1);
                enc.template code<false, true>(lo, hi - lo, k);
            }
            cur = nxt;
        }
    } else {
        for (u32 i = 0; i < maxlen; ++i) {
            if (i < len) {
                const u32 b = in[i];
                const u32 lo = tab.get(b), hi = tab.get(b + 1);
                enc.template code<false, true>(lo, hi - lo, k);
            }
        }
    }

    if (live) {
        if (enc.low == 0xFFFFFFFFu) enc.acc += 1; // cpprcoder.h:439-443: bump the held byte, pending 0xFF -> 0x00
        const u32 bytes = enc.finish() + (RCX_STATIC_HEADER - 4);
        sizes[blk] = enc.overflow ? (u32)slot : bytes;
        if (enc.overflow) rcx_flag(status, RCX_ST_CAPACITY, rcx_id(g, blk));
    }
}

// ===========================================================================
// Static encode, pass 1, three waves per 64 blocks: the five-wave adaptive encoder (rcx_enc_mc5_k, rcx_mc.hpp)
// without its model waves -- the table does not change while coding.  wave 0 = arithmetic (EncLane::arith with
// full 32-bit multiplies), wave 1 = writer (StagedWriter: words through LDS rings), wave 2 = table lookups for
// the next chunk + the drain of the rings.  The histogram (cpprcoder.h:543-571) is counted by all three waves
// with LDS atomics for the first 65535 symbols of a block, where its 16-bit squeeze cannot fire.
// A carry through more output bytes than the rings keep back marks the block in `redo` for rcx_enc_static_k.
// ===========================================================================
#define RCX_ST3_THREADS 192
#define RCX_ST3_LDS_DW (RCX_STATIC_LDS_DW + 4 * RCX_MC_RING_U4 + RCX_MC5_RING2_DW + RCX_LANES + RCX_MC5_OUT_DW)

// WIDE: full 32-bit multiplies.  With a total below 256, t = range / total can exceed 24 bits; from 256 on it cannot,
// and cum and count never do (total <= 2^24), so the 24-bit multiplies of the adaptive coder are exact.
template <bool FULL, bool WIDE>
__device__ __forceinline__ void rcx_static3_pipeline(u32 wave, u32 lane, u32 len, u32 nchunks, const u8* in, const StaticTable& tab,
                                                     U4* ring, u32* ring2, EncLane& enc, const DivEntry& kdiv, StagedWriter& wr,
                                                     u32* out_pos, u32& drained, u8* payload, u32 cap, bool live)
{
    U4 piece_ahead;
    piece_ahead.x = piece_ahead.y = piece_ahead.z = piece_ahead.w = 0;
    if (FULL && wave == 2 && nchunks > 0) piece_ahead = *reinterpret_cast<const U4*>(in);
    for (u32 k = 0; k <= nchunks + 1; ++k) {
        if (wave == 0) {
            // ---- arithmetic: chunk k-1 ----
            if (k >= 1 && k <= nchunks) {
                const u32 i0 = (k - 1) * RCX_MC_CHUNK;
                const U4* rs = ring + ((k - 1) & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;
                u32* ws2 = ring2 + ((k - 1) & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;
                U4 e_next = rs[0];
                u32 rec_even = 0;
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    const U4 e = e_next;
                    if (s + 1 < RCX_MC_CHUNK) e_next = rs[(s + 1) * RCX_LANES];
                    u32 rec = 0;
                    if (FULL || i0 + s < len) rec = enc.template arith<WIDE>(e.x, e.w, kdiv); // cpprcoder.h:402-408
                    if ((s & 1u) == 0) rec_even = rec; // (two symbols' records per LDS instruction: see rcx_mc5_pipeline)
                    else {
                        ws2[(s - 1) * RCX_LANES] = rec_even;
                        ws2[s * RCX_LANES] = rec;
                    }
                }
            }
        } else if (wave == 1) {
            RCX_MC_WRITER_STAGE(k, ring2, wr, out_pos) // chunk k-2
        } else {
            // ---- drain (rcx_mc.hpp: the reads here, the stores between the wait for this chunk's input and the request
            // for the next chunk's) ----
            u32 drain_p;
            RcxU4Unaligned drain_piece;
            RCX_MC_DRAIN_READ(drain_p, drain_piece, out_pos, wr, drained)
            auto drain_store = [&]() { RCX_MC_DRAIN_STORE(drain_p, drain_piece, wr, payload, drained, cap, live) };
            if (k >= nchunks) drain_store();
            // ---- lookups: chunk k ----
            if (k < nchunks) {
                const u32 i0 = k * RCX_MC_CHUNK;
                U4* ws = ring + (k & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;
                U4 piece;
                if (FULL) {
                    piece = piece_ahead;
                    asm volatile("" ::"v"(piece.x), "v"(piece.y), "v"(piece.z), "v"(piece.w)); // (the input has arrived before a store is issued)
                }
                drain_store();
                if (FULL) {
                    if (k + 1 < nchunks) piece_ahead = *reinterpret_cast<const U4*>(in + i0 + RCX_MC_CHUNK);
                } else {
                    u32 w[4] = {0, 0, 0, 0};
                    for (u32 s = 0; s < RCX_MC_CHUNK; ++s)
                        if (i0 + s < len) w[s >> 2] |= (u32)in[i0 + s] << (8 * (s & 3));
                    piece.x = w[0];
                    piece.y = w[1];
                    piece.z = w[2];
                    piece.w = w[3];
                }
                u32 b = rcx_byte_of(piece, 0);
                u32 lo = tab.get(b), hi = tab.get(b + 1);
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    const u32 lo_s = lo, hi_s = hi;
                    if (s + 1 < RCX_MC_CHUNK) {
                        b = rcx_byte_of(piece, s + 1);
                        lo = tab.get(b);
                        hi = tab.get(b + 1);
                    }
                    u32* e = reinterpret_cast<u32*>(&ws[s * RCX_LANES]);
                    e[0] = lo_s;        // cum
                    e[3] = hi_s - lo_s; // count
                }
            }
        }
        rcx_lds_barrier();
    }
}

template <class G = RcxBlocks>
__global__ __launch_bounds__(RCX_ST3_THREADS) void rcx_enc_static3_k(const u8* __restrict__ src, u64 n, u32 block, u64 nblocks,
                                                                    u8* __restrict__ slots, u64 slot, u32* __restrict__ sizes,
                                                                    u32* status, u32* __restrict__ redo, u32 lanes_used, const G g = G())
{
    __shared__ __attribute__((aligned(RCX_OUT_RING_BYTES))) u32 lds_all[RCX_ST3_LDS_DW]; // (McOutput first: RCX_MC_OUTPUT)
    static_assert(__alignof__(lds_all) % RCX_OUT_RING_BYTES == 0, "the output ring's place in LDS");
    u32* lds = lds_all + RCX_MC_OUTPUT_AT_DW + RCX_MC_OUTPUT_DW;
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool in_use = lane < lanes_used; // see rcx_enc_mc5_k
    const u64 blk = in_use ? (u64)blockIdx.x * lanes_used + lane : nblocks;
    RCX_ENTRY(g, blk, nblocks, n, block);
    RCX_ENTRY_SLOTS(g, blk, slots, slot);
    const u8* in = src + at;
    StaticTable tab{lds + lane};
    U4* ring = reinterpret_cast<U4*>(lds + RCX_STATIC_LDS_DW); // 16-byte aligned: RCX_STATIC_LDS_DW = 257 * 64 dwords, behind 68 * 64
    u32* ring2 = reinterpret_cast<u32*>(ring + RCX_MC_RING_U4);
    RCX_MC_OUTPUT(oq, lds_all + RCX_MC_OUTPUT_AT_DW);

    const u32 maxlen = rcx_wave_max(len);
    // (RCX_ALL_FULL, but for the lanes that carry no block: they do not count)
    const bool full = !G::items && __all(!in_use || (live && len == block)) && (block % 16u == 0) && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    const u32 nchunks = (maxlen + RCX_MC_CHUNK - 1) / RCX_MC_CHUNK;

    // ---- count(), cpprcoder.h:543-571 ----
    for (u32 i = wave; i <= 256; i += 3) tab.set(i, 0);
    {
        U4 z; // the ring entries' two middle dwords stay 0: the arithmetic wave adds x + y + z
        z.x = z.y = z.z = z.w = 0;
        for (u32 i = wave; i < 2 * RCX_MC_CHUNK; i += 3) ring[i * RCX_LANES + lane] = z;
    }
    rcx_lds_barrier();
    // a count can only be 0xFFFF before its increment once 65535 earlier symbols exist: no squeeze test before
    const u32 easy = maxlen < 65535u ? maxlen : 65535u;
    const u32 easy16 = full ? easy & ~15u : 0u;
    for (u32 i = 16 * wave; i < easy16; i += 48) {
        const U4 piece = *reinterpret_cast<const U4*>(in + i);
#pragma unroll
        for (u32 s = 0; s < 16; ++s) tab.inc(rcx_byte_of(piece, s));
    }
    rcx_lds_barrier();
    if (easy < maxlen) {
        // Past symbol 65535.  If no count can reach 0xFFFF before the block ends (largest count so far + the
        // symbols left: every wave computes the same answer from the same table) the three waves go on as
        // before; otherwise the order matters and wave 0 counts the rest alone, in order, with the test.
        const u32 mx = rcx_static_max_count(tab);
        const bool calm = __all(mx + (len > easy16 ? len - easy16 : 0u) < 0xFFFFu);
        rcx_lds_barrier(); // (wave 0 may not start changing the table while another wave still reads it)
        if (wave == 0) {
            for (u32 i = easy16; i < easy; ++i)
                if (i < len) tab.inc(in[i]);
        }
        if (calm && full) {
            const u32 from = (easy + 15u) & ~15u; // 65536
            const u32 to16 = maxlen & ~15u;
            if (wave == 0)
                for (u32 i = easy; i < from && i < maxlen; ++i) tab.inc(in[i]);
            for (u32 i = from + 16 * wave; i < to16; i += 48) {
                const U4 piece = *reinterpret_cast<const U4*>(in + i);
#pragma unroll
                for (u32 s = 0; s < 16; ++s) tab.inc(rcx_byte_of(piece, s));
            }
            if (wave == 0)
                for (u32 i = (to16 > from ? to16 : from); i < maxlen; ++i) tab.inc(in[i]);
        } else if (wave == 0) {
            if (full) {
                const u32 from = (easy + 15u) & ~15u;
                rcx_static_count_checked<false>(tab, in, easy, from < maxlen ? from : maxlen, len);
                if (from < maxlen) rcx_static_count_checked<true>(tab, in, from, maxlen, len);
            } else {
                rcx_static_count_checked<false>(tab, in, easy, maxlen, len);
            }
        }
    } else if (wave == 0) {
        for (u32 i = easy16; i < easy; ++i)
            if (i < len) tab.inc(in[i]);
    }
    rcx_lds_barrier();

    // ---- header: u32 LE n + 256 u16 counts (cpprcoder.h:386-397, :604-619) ----
    u8* wave_slots = slots + (u64)blockIdx.x * lanes_used * slot;
    EncLane enc;
    enc.idle(wave_slots);
    StagedWriter wr;
    wr.begin(oq.ring, oq.dummy, lane);
    u32 drained = 0;
    if (wave == 1) {
        if (live) {
            enc.begin(wave_slots, lane * (u32)slot, (u32)slot, len);
            u32* hdr = reinterpret_cast<u32*>(wave_slots + lane * (u32)slot + 4);
            for (u32 i = 0; i < 256; i += 2) hdr[i >> 1] = (tab.get(i) & 0xFFFFu) | (tab.get(i + 1) << 16);
            enc.off += RCX_STATIC_HEADER - 4;
            enc.cap -= RCX_STATIC_HEADER - 4;
        }
        oq.pos[lane] = 0;
    }
    rcx_lds_barrier();
    if (wave == 2) (void)tab.accumulate(); // cpprcoder.h:573-583; entry 256 = total
    rcx_lds_barrier();
    const u32 total = tab.get(256);
    const DivEntry k = rcx_make_div_entry(total ? total : 1u);
    enc.range = 0xFFFFFFFFu; // cpprcoder.h:382

    u8* payload = wave_slots + (u64)lane * slot + RCX_STATIC_HEADER;
    const u32 cap = (((u32)slot - 4) & ~3u) - (RCX_STATIC_HEADER - 4);
    const bool narrow = __all(total >= 256u); // every wave sees the same table
    if (full && narrow) rcx_static3_pipeline<true, false>(wave, lane, len, nchunks, in, tab, ring, ring2, enc, k, wr, oq.pos, drained, payload, cap, live);
    else if (full) rcx_static3_pipeline<true, true>(wave, lane, len, nchunks, in, tab, ring, ring2, enc, k, wr, oq.pos, drained, payload, cap, live);
    else rcx_static3_pipeline<false, true>(wave, lane, len, nchunks, in, tab, ring, ring2, enc, k, wr, oq.pos, drained, payload, cap, live);

    RCX_MC_CLOSE_HANDOVER(wave, 2, oq, enc, drained);
    if (wave == 1 && live) {
        RCX_MC_CLOSE_FLUSH(oq, wr, enc, payload, cap)
        if (enc.low == 0xFFFFFFFFu) enc.acc += 1; // cpprcoder.h:439-443
        const u32 bytes = enc.finish() + (RCX_STATIC_HEADER - 4);
        RCX_MC_CLOSE_REPORT(bytes, enc, wr, g, blk, slot, sizes, status, redo);
    } else if (wave == 1 && blk < nblocks) {
        redo[blk] = 0;
    }
}

// ===========================================================================
// Static decode
// ===========================================================================
// STREAM = the single-stream entry point: one block whose symbol count n the host took from the header;
// track[0] = first symbol whose renormalisation ran out of input (cpprcoder.h:506-509), or 0xFFFFFFFF.
template <bool STREAM, class G = RcxBlocks>
__global__ __launch_bounds__(64) void rcx_dec_static_k(const u8* __restrict__ comp, u64 comp_size, const u64* __restrict__ offsets, u64 nblocks,
                                                       u32 block, u64 n, u8* __restrict__ dst, u32* status, u32* track,
                                                       const u32* __restrict__ only, const G g = G())
{
    __shared__ u32 lds[RCX_STATIC_LDS_DW + RCX_RING_DW * RCX_LANES];
    const u32 lane = threadIdx.x;
    const u64 blk = (u64)blockIdx.x * RCX_LANES + lane;
    // second pass behind rcx_dec_static_quad_k: only the blocks it marked (none, on valid input)
    RCX_ENTRY_ONLY(g, blk, nblocks, n, block, only);
    StaticTable tab{lds + lane};
    u32* ring_col = lds + RCX_STATIC_LDS_DW + lane;

    DecLane dec;
    u64 stream_len = 0;
    u32 total = 1;
    for (u32 i = 0; i <= 256; ++i) tab.set(i, 0);
    if (live) {
        // cpprcoder.h:474-493: at least the header, one more byte, then 5 bytes for the lead-in and low
        RCX_STREAM(g, blk, offsets);
        const u8* s = comp + s0;
        bool good = RCX_STREAM_OK(comp_size, RCX_STATIC_HEADER + 5);
        if (good) {
            const u32 declared = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
            good = STREAM || declared == len;
        }
        if (good) {
            for (u32 i = 0; i < 256; ++i) tab.set(i, (u32)s[4 + 2 * i] | ((u32)s[5 + 2 * i] << 8)); // :585-602
            total = tab.accumulate();
            good = total != 0; // the reference would divide by zero
        }
        if (good) {
            // DecLane::begin expects 4 size bytes + 4 bytes of low; the static stream has its lead-in byte
            // in between (low = bytes[1..4], cpprcoder.h:494-498): start it 3 bytes early and fix low up.
            const u8* h = s + RCX_STATIC_HEADER - 3;
            dec.begin(h, comp + s1, ring_col);
            dec.low = ((u32)h[4] << 24) | ((u32)h[5] << 16) | ((u32)h[6] << 8) | (u32)h[7];
            dec.range = 0xFFFFFFFFu;
        } else {
            if (!STREAM) rcx_flag(status, RCX_ST_CORRUPT, rcx_id(g, blk));
            live = false;
            len = 0;
        }
    }
    if (!live) {
        dec.idle(comp, ring_col);
        total = 1;
    }
    const DivEntry k = rcx_make_div_entry(total);
    // cum[16], cum[32], ..., cum[240] never change: keep them in registers for the first search level
    u32 coarse[15];
#pragma unroll
    for (u32 q = 0; q < 15; ++q) coarse[q] = tab.get(16 * (q + 1));

    const u32 maxlen = rcx_wave_max(len);
    const bool full = !STREAM && RCX_ALL_FULL(g, block, dst);
    u8* out = dst + at;
    bool bad = false;
    u32 short_at = 0xFFFFFFFFu;

    if (full) {
        for (u32 i = 0; i < maxlen; i += 16) {
            u32 word[4] = {0, 0, 0, 0};
            dec.topup();
#pragma unroll
            for (u32 s = 0; s < 16; ++s) {
                const u32 sym = rcx_static_symbol(dec, tab, coarse, k, total, bad); // (rcx_lane.hpp)
                word[s >> 2] |= sym << (8 * (s & 3));
            }
            U4 o;
            o.x = word[0];
            o.y = word[1];
            o.z = word[2];
            o.w = word[3];
            *reinterpret_cast<U4*>(out + i) = o;
        }
    } else {
        for (u32 i = 0; i < maxlen; ++i) {
            if ((i & 15u) == 0) dec.topup();
            if (i < len) {
                out[i] = (u8)rcx_static_symbol(dec, tab, coarse, k, total, bad);
                if (STREAM && short_at == 0xFFFFFFFFu && (bad || dec.taken() + (RCX_STATIC_HEADER - 3) > stream_len)) short_at = i;
            }
        }
    }
    // cpprcoder.h:506-509: running out of input inside the renormalisation is a failure
    if (STREAM) {
        if (lane == 0) track[0] = live ? short_at : 0u;
    } else if (live && (bad || dec.taken() + (RCX_STATIC_HEADER - 3) > stream_len)) {
        rcx_flag(status, RCX_ST_CORRUPT, rcx_id(g, blk));
    }
}

// ===========================================================================
// Static decode, 4 lanes per block: rcx_dec_quad_k's machinery (rcx_quad.hpp) with less to do per
// symbol -- the table never changes.  The block's 256 cumulative counts cum[1..256] (cpprcoder.h:573-583)
// sit in LDS as 16 nodes of 16 entries in the same bank-conflict-free table groups; lane j keeps the
// upper bounds of its four nodes, cum[16(4j+1)] .. cum[16(4j+4)], in registers for the whole block.
// find() (cpprcoder.h:521-535) counts the entries cum[1..255] that are <= low/t; in the scaled domain
// (cum*t <= low: every product is <= total*t <= range < 2^32) that is round 1 = the node bounds that do not
// borrow in low - bound*t, round 2 = the same over the node's 16 entries, read as they are (they are already
// cumulative: no scan).  low - cum[c]*t is the unsigned minimum of the differences, and the new range
// (cum[c+1] - cum[c])*t is minimum - maximum (mod 2^32), as in the adaptive decoder.  No update.
// The reference normalises AFTER a symbol (cpprcoder.h:500-517); with range = 0xFFFFFFFF at the start that is
// the same as normalising before the next one, plus once after the last.
// A stream whose target runs past the table or that names a symbol of count 0 (damaged input) is marked in
// `redo` and decoded by rcx_dec_static_k, which reports it the way the reference fails.
// ===========================================================================
template <int WAVES, class G = RcxBlocks>
__global__ __launch_bounds__(64 * WAVES) void rcx_dec_static_quad_k(const u8* __restrict__ comp, u64 comp_size, const u64* __restrict__ offsets,
                                                                    u64 nblocks, u32 block, u64 n, u8* __restrict__ dst,
                                                                    u32* status, u32* __restrict__ redo, u32 quads_used, const G g = G())
{
    __shared__ __attribute__((aligned(256))) u8 lds_all[WAVES * RCX_QUAD_LDS_BYTES];
    RCX_QUAD_SEAT(seat, WAVES, quads_used, lds_all, g, nblocks, n, block); // (as rcx_dec_quad_k)

    QuadInput in;
    u64 stream_len = 0;
    u32 U1 = 1, U2 = 2, U3 = 3, U4_ = 4, total = 4;
    if (live) {
        // cpprcoder.h:474-493: at least the header, one more byte, then 5 bytes for the lead-in and low
        RCX_STREAM(g, seat.blk, offsets);
        const u8* s = comp + s0;
        bool good = RCX_STREAM_OK(comp_size, RCX_STATIC_HEADER + 5);
        if (good) {
            const u32 declared = (u32)s[0] | ((u32)s[1] << 8) | ((u32)s[2] << 16) | ((u32)s[3] << 24);
            good = declared == len;
        }
        if (good) {
            // cpprcoder.h:585-602 + :573-583: lane j takes the counts of symbols 64j .. 64j+63
            const u8* cs = s + 4 + 128 * seat.j;
            u32 mysum = 0;
            for (u32 i = 0; i < 64; ++i) mysum += (u32)cs[2 * i] | ((u32)cs[2 * i + 1] << 8);
            u32 run = rcx_quad_excl_scan(mysum, (seat.j & 1u) ? ~0u : 0u, (seat.j & 2u) ? ~0u : 0u);
            for (u32 i = 0; i < 64; ++i) {
                run += (u32)cs[2 * i] | ((u32)cs[2 * i + 1] << 8);
                // entry e = 64j + i + 1 = cum[e] lives in node (e-1)/16 at position (e-1)%16
                reinterpret_cast<u32*>(seat.mine + (4 * seat.j + (i >> 4)) * 256)[i & 15u] = run;
                if (i == 15) U1 = run;
                if (i == 31) U2 = run;
                if (i == 47) U3 = run;
            }
            U4_ = run;
            total = rcx_dpp<0xFF>(U4_); // quad_perm [3,3,3,3]: cum[256]
            good = total != 0;          // the reference would divide by zero
        }
        if (good) {
            // QuadInput::begin expects 4 size bytes + 4 bytes of low; the static stream has its lead-in byte in
            // between (low = bytes[1..4] after the header, cpprcoder.h:494-498): start it 3 bytes early
            in.begin(s + RCX_STATIC_HEADER - 3, comp + s1, seat.ring, seat.parked + 3);
            in.range = 0xFFFFFFFFu;
        } else {
            RCX_QUAD_FAIL(seat, g, status)
        }
    }
    if (!live) {
        in.idle(comp, seat.ring, seat.parked + 3);
        U1 = 1, U2 = 2, U3 = 3, U4_ = 4, total = 4;
        U4 v;
        v.x = v.y = v.z = v.w = 4;
        for (u32 q = 0; q < 16; ++q) seat.leaves[q * 16] = v;
    }
    {
        U4 v; // the scratch row ("node 16", reached only by a target past the table)
        v.x = v.y = v.z = v.w = 0;
        seat.leaves[16 * 16] = v;
    }
    const DivEntry k = rcx_make_div_entry(total);
    const u64 kadd = k.add;

    const u32 maxlen = rcx_wave_max(len);
    const bool full = RCX_ALL_FULL(g, block, dst);
    u8* out = dst + at;
    const bool leader = live && seat.in_use && seat.j == 0;
    const u32 leaves_lds = (u32)reinterpret_cast<uintptr_t>(seat.leaves);
    const u32 ring_lds = (u32)reinterpret_cast<uintptr_t>(seat.ring);
    u32 worst_node = 0;            // 16 = a target past the table
    u32 least_range = 0xFFFFFFFFu; // 0 = a symbol of count 0

    // One symbol (instruction sequences as in rcx_dec_quad_k: no compare result or DPP source is used before two
    // other instructions have been issued).  Every lane of the quad ORs the symbol into WORD at bit SHIFT.
    // (as in rcx_dec_quad_k, what the coder state does not need -- the symbol's byte, the watch on the smallest range -- is
    // made by the NEXT symbol behind its leaf read: HP = 1, PWORD / PSHIFT = the earlier symbol's word and bit position;
    // RCX_SQUAD_FINISH makes the last one)
    u32 p_nd_ = 0, p_nb_ = 0, p_rg_ = 0xFFFFFFFFu;
#define RCX_SQ_PREV_0
#define RCX_SQ_PREV_1 "\n\tv_lshl_add_u32 %[ps], %[pnd], 4, %[pnb]\n\t"                                             \
                      "v_min_u32 %[lr], %[lr], %[prg]\n\t"                                                           \
                      "v_lshl_or_b32 %[pword], %[ps], %[psh], %[pword]"
#define RCX_SQUAD_FINISH(WORD, SHIFT)                                                                      \
    {                                                                                                      \
        (WORD) |= ((p_nd_ << 4) + p_nb_) << (SHIFT);                                                       \
        least_range = least_range < p_rg_ ? least_range : p_rg_;                                           \
    }
#define RCX_SQUAD_SYMBOL(HP, PWORD, PSHIFT)                                                                \
    {                                                                                                      \
        const u32 k8_ = rcx_clz(in.range) & 0x18u; /* cpprcoder.h:511-516, for the previous symbol */      \
        in.low = (u32)((((u64)in.low << 32) | in.n4) << k8_ >> 32);                                        \
        in.range <<= k8_;                                                                                  \
        const u32 t_ = (u32)(((u64)in.range * k.mul + kadd) >> 32) >> (k.shift & 31u); /* :502 */          \
        const u32 a1_ = U1 * t_, a2_ = U2 * t_, a3_ = U3 * t_, a4_ = U4_ * t_;                             \
        u32 node_, rem_, ro_, la_, x1_, x2_, x3_, x4_;                                                     \
        u64 c1_, c2_, c3_, c4_;                                                                            \
        /* (ordered as in rcx_dec_quad_k: the node index first -- the leaf read waits for it --, the next symbol's stream  \
           bytes asked for before it, the remainder's steps across the quad and the stream bytes' extraction behind it) */ \
        asm volatile("v_sub_co_u32_e64 %[x1], %[c1], %[low], %[a1]\n\t"                                    \
                     "v_sub_co_u32_e64 %[x2], %[c2], %[low], %[a2]\n\t"                                    \
                     "v_sub_co_u32_e64 %[x3], %[c3], %[low], %[a3]\n\t"                                    \
                     "v_sub_co_u32_e64 %[x4], %[c4], %[low], %[a4]\n\t"                                    \
                     "v_subb_co_u32_e64 %[nd], %[c1], 4, 0, %[c1]\n\t"                                     \
                     "v_subb_co_u32_e64 %[nd], %[c2], %[nd], 0, %[c2]\n\t"                                 \
                     "v_subb_co_u32_e64 %[nd], %[c3], %[nd], 0, %[c3]\n\t"                                 \
                     "v_subb_co_u32_e64 %[nd], %[c4], %[nd], 0, %[c4]\n\t"                                 \
                     "v_add_u32 %[bp], %[bp], %[k8]\n\t"                                                   \
                     "v_bfe_u32 %[ro], %[bp], 5, 5\n\t"                                                    \
                     "v_lshl_add_u32 %[ro], %[ro], 2, %[rb]"                                                \
                     : [nd] "=&v"(node_), [ro] "=&v"(ro_), [bp] "+v"(in.bp8),                               \
                       [x1] "=&v"(x1_), [x2] "=&v"(x2_), [x3] "=&v"(x3_), [x4] "=&v"(x4_),                 \
                       [c1] "=&s"(c1_), [c2] "=&s"(c2_), [c3] "=&s"(c3_), [c4] "=&s"(c4_)                  \
                     : [low] "v"(in.low), [a1] "v"(a1_), [a2] "v"(a2_), [a3] "v"(a3_), [a4] "v"(a4_),      \
                       [k8] "v"(k8_), [rb] "v"(ring_lds));                                                 \
        {                                                                                                  \
            const RcxLdsU32* at_ = reinterpret_cast<const RcxLdsU32*>(ro_); /* for the next symbol */      \
            in.w0 = at_[0];                                                                                \
            in.w1 = at_[1];                                                                                \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        asm volatile("v_add_u32_dpp %[nd], %[nd], %[nd] " RCX_QP1                                          \
                     "v_min3_u32 %[rm], %[x1], %[x2], %[x3]\n\t"                                           \
                     "v_min3_u32 %[rm], %[rm], %[x4], %[low]\n\t"                                          \
                     "v_add_u32_dpp %[nd], %[nd], %[nd] " RCX_QP2                                          \
                     "v_lshl_add_u32 %[la], %[nd], 8, %[lvb]"                                              \
                     : [nd] "+v"(node_), [rm] "=&v"(rem_), [la] "=&v"(la_)                                  \
                     : [low] "v"(in.low), [x1] "v"(x1_), [x2] "v"(x2_), [x3] "v"(x3_), [x4] "v"(x4_),      \
                       [lvb] "v"(leaves_lds));                                                             \
        const RcxV4 l_ = *reinterpret_cast<const RcxLdsV4*>(la_);                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        asm volatile("v_min_u32_dpp %[rm], %[rm], %[rm] " RCX_QP1                                          \
                     "v_max_u32 %[wn], %[wn], %[nd]"                                                       \
                     : [rm] "+v"(rem_), [wn] "+v"(worst_node)                                               \
                     : [nd] "v"(node_));                                                                   \
        u32 ps_;                                                                                           \
        asm volatile("v_alignbit_b32 %[n4], %[w1], %[w0], %[bp]\n\t" /* the 4 bytes at bp8 ... */           \
                     "v_min_u32_dpp %[rm], %[rm], %[rm] " RCX_QP2                                          \
                     "v_perm_b32 %[n4], %[n4], %[n4], %[swap]"      /* ... first one on top */              \
                     RCX_SQ_PREV_##HP                                                                      \
                     : [rm] "+v"(rem_), [n4] "=&v"(in.n4), [ps] "=&v"(ps_), [lr] "+v"(least_range), [pword] "+v"(PWORD) \
                     : [w0] "v"(in.w0), [w1] "v"(in.w1), [bp] "v"(in.bp8), [swap] "s"(0x00010203u),        \
                       [pnd] "v"(p_nd_), [pnb] "v"(p_nb_), [prg] "v"(p_rg_), [psh] "n"(PSHIFT));           \
        const u32 q1_ = l_.x * t_, q2_ = l_.y * t_, q3_ = l_.z * t_, q4_ = l_.w * t_;                      \
        RCX_QUAD_ROUND2_CUM(in.low, q1_, q2_, q3_, q4_);                                                   \
        in.low = lo_;   /* :504 */                                                                         \
        in.range = rg_; /* :505 */                                                                         \
        p_nd_ = node_;  /* the symbol = node << 4 | nb, in all four lanes */                                \
        p_nb_ = nb_;                                                                                       \
        p_rg_ = rg_;                                                                                       \
    }

    if (full) {
        U4 o_last; // (RCX_QUAD_PARKED_*, rcx_quad.hpp)
        o_last.x = o_last.y = o_last.z = o_last.w = 0;
        for (u32 i0 = 0; i0 < maxlen; i0 += 16) {
            in.topup();
            RCX_QUAD_PARKED_FLUSH(i0, seat.parked, o_last, G::items)
            u32 w0_ = 0, w1_ = 0, w2_ = 0, w3_ = 0;
            RCX_QUAD_16_SYMBOLS(RCX_SQUAD_SYMBOL, RCX_SQUAD_FINISH)
            U4 o;
            o.x = w0_;
            o.y = w1_;
            o.z = w2_;
            o.w = w3_;
            RCX_QUAD_PARKED_PUT(o, seat.parked, o_last);
        }
        RCX_QUAD_PARKED_END(maxlen, seat.parked, o_last, G::items)
    } else {
        RCX_QUAD_TAIL(0u, , RCX_SQUAD_SYMBOL, RCX_SQUAD_FINISH, )
    }
#undef RCX_SQUAD_SYMBOL
#undef RCX_SQUAD_FINISH
#undef RCX_SQ_PREV_0
#undef RCX_SQ_PREV_1
    // the normalisation after the last symbol (it decides whether the input was long enough, cpprcoder.h:506-509)
    in.bp8 += rcx_clz(in.range) & 0x18u;
    const bool marked = live && (worst_node >= 16u || least_range == 0);
    if (leader && !marked && in.taken() + (RCX_STATIC_HEADER - 3) > stream_len) rcx_flag(status, RCX_ST_CORRUPT, rcx_id(g, seat.blk));
    RCX_QUAD_MARK_REDO(seat, redo, nblocks, marked);
}
