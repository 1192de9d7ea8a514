// rcx_mc.hpp -- the multi-wave range encoders' machinery, and the adaptive one itself:
//   the rings between the waves, rcx_lds_barrier, StagedWriter (the byte writer whose words leave through LDS), the
//   drain of its rings, the output-ring layout (McOutput), the writer and drain stages and the closing stage
//   rcx_enc_mc5_k    adaptive encode, seven waves per 64 blocks (model x4 / arithmetic / writer / drain)
// rcx_enc_static3_k (rcx_static.hpp) is built on the same machinery.
#pragma once
// included by rcx_kernels.hpp behind rcx_quad.hpp (uses rcx_flag, rcx_wave_max, rcx_byte_of; RcxV4, RcxLdsU32 from rcx_quad.hpp)

// The multi-wave encoders: 16 symbols per pipeline step, double-buffered rings between the waves
#define RCX_MC_CHUNK 16
#define RCX_MC_THREADS 256
#define RCX_MC_RING_U4 (2 * RCX_MC_CHUNK * RCX_LANES)
#define RCX_MC_LDS_U4 (RCX_LDS_U4 + RCX_MC_RING_U4)

__device__ __forceinline__ void rcx_lds_barrier()
{
    // LDS hand-off between the waves of one workgroup: drain this wave's LDS operations, then
    // meet.  Deliberately not __syncthreads(): that also waits for vmcnt(0) and would stall the
    // coder wave on its own in-flight global stores every chunk.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#if defined(RCX_STAMP) /* diagnostic build only (tools/diag/stamp_encode.py) */
static __device__ unsigned long long rcx_stamp_out[16];
#define rcx_stamp_wait stamp_wait_
#endif

// ===========================================================================
// Encode, pass 1, five-wave split ("MC5"): as rcx_enc_mc_k, with the coder itself cut in two
// (EncLane::arith / EncLane::emit): the interval arithmetic (state low, range) and the byte
// writer (state acc / nacc8 / pos, the global stores) are separate waves connected by a second
// LDS ring of one record per symbol.  Three pipeline stages, one chunk apart:
//   waves M1..M3 (model, chunk k) -> wave A (arithmetic, chunk k-1) -> wave W (writer, chunk k-2)
// Five waves on four SIMDs: the two lightest (A and the level-1 model wave) are meant to share one.
//
// The writer does not store to global memory: scattered 4-byte stores under an EXEC mask were its most
// expensive step.  Its bytes go to a per-block ring in LDS (StagedWriter: a window of the newest eight bytes mirrored
// there, two words a symbol), and the level-1 model wave drains the rings once per chunk with 16-byte stores (the leaf
// wave or the writer itself measured no better: a drain costs its wave the same wherever it runs).
// The drain keeps the newest RCX_OUT_MARGIN bytes back, so that a carry that runs through more than the newest four
// bytes (cpprcoder.h:767-781) is resolved in LDS; a run of 0xFF bytes longer than that margin cannot be,
// and such a block is marked in `redo` and encoded again by rcx_enc_adaptive_k.
// Level 3 of the model (one group per block) lives in registers of a wave of its own, the other levels in LDS.
// ===========================================================================
// The kernel's wave ROLES are numbered 0 arithmetic, 1 writer, 2 model level 2, 3 model leaf level, 4 model level 1,
// 5 drain (a wave that does nothing else), 6 model level 3.  A workgroup's wave i runs on SIMD i mod 4, and a wave that
// is alone on its SIMD pays 4 cycles for every wait and scalar instruction and 12-28 for every LDS instruction, which a
// second wave hides.  The hardware's waves 1 and 3 swap roles, so that the pairs are arithmetic + level 1, leaf + drain
// and level 2 + level 3; the writer is alone.
#define RCX_DRAIN_WAVE 5
#define RCX_L3_WAVE 6
#define RCX_MC5_THREADS 448
// (Both are switches for measuring other pairings, DESIGN.md 3.2: with seven waves a SIMD has two at the most.)
#if !defined(RCX_MC5_ROLES)
#define RCX_MC5_ROLES 0x6541230u /* one hex digit per hardware wave, wave 0 lowest */
#endif
#if !defined(RCX_MC5_PRIO)
#define RCX_MC5_PRIO 0x10u /* the roles that run at s_setprio 1 (rcx_mc5_pipeline), one bit each: level 1 */
#endif
#define RCX_MC5_ROLE(HW) (((u32)RCX_MC5_ROLES >> (4u * (HW))) & 15u)
// The ring between the model waves and the arithmetic wave: four dwords per symbol and lane.  Kept as 16 contiguous
// bytes per lane (one ds_read_b128 for the arithmetic wave; the model waves' 4-byte stores hit each bank four times)
// or, RCX_RING_PLANAR=1, as four dword planes (conflict-free stores, two ds_read2st64_b32).
#if !defined(RCX_RING_PLANAR)
#define RCX_RING_PLANAR 0
#endif
#if !defined(RCX_MODEL_AHEAD)
#define RCX_MODEL_AHEAD 2 /* symbols the model waves' LDS reads and updates run ahead of their sums */
#endif
#if !defined(RCX_ARITH_AHEAD)
#define RCX_ARITH_AHEAD 1 /* symbols the arithmetic wave's ring and divisor reads run ahead */
#endif
#if RCX_RING_PLANAR
#define RCX_RING_LANE 1
#define RCX_RING_AT(s, f) ((4 * (s) + (f)) * RCX_LANES)
#else
#define RCX_RING_LANE 4
#define RCX_RING_AT(s, f) (4 * (s) * RCX_LANES + (f))
#endif
#define RCX_MC5_RING2_DW (2 * RCX_MC_CHUNK * RCX_LANES)
#define RCX_OUT_RING_WORDS 64 /* per block: 256 bytes of output waiting in LDS */
#define RCX_OUT_MARGIN 32     /* bytes kept back from the drain */
#define RCX_MC5_OUT_DW (RCX_OUT_RING_WORDS * RCX_LANES + 3 * RCX_LANES)
// The writer forms a ring word's LDS address as (running position bits & RCX_OUT_SLOT_MASK) | the lane's address in slot 0
// (StagedWriter::emit): an OR, so the ring begins at a multiple of its own size in the workgroup's LDS.  Both kernels put
// McOutput first in an array aligned to it (RCX_MC_OUTPUT_AT_DW).
#define RCX_OUT_RING_BYTES (RCX_OUT_RING_WORDS * RCX_LANES * 4)
#define RCX_OUT_SLOT_MASK ((RCX_OUT_RING_WORDS - 1u) * RCX_LANES * 4u) /* 0x3F00: slots are 256 bytes, bits 8-13 */
#define RCX_MC_OUTPUT_AT_DW 0                                            /* where McOutput begins in either kernel's LDS array */
#define RCX_MC_OUTPUT_DW (RCX_LANES + RCX_MC5_OUT_DW)                    /* ring, slot 64, final_low, pos, drained */
static_assert(RCX_OUT_RING_BYTES == 16384 && RCX_OUT_SLOT_MASK == 0x3F00u, "the output ring: 64 slots of 256 bytes");
static_assert((RCX_MC_OUTPUT_AT_DW * 4) % RCX_OUT_RING_BYTES == 0, "the output ring starts at a multiple of 16 KiB");
static_assert(RCX_MC_OUTPUT_DW % 4 == 0, "what follows McOutput stays 16-byte aligned");
// The level-3 wave's sums: a fifth value per symbol and lane, in a dword plane of its own beside the ring (the ring's record
// stays the 16 bytes per lane that the arithmetic wave reads at once), double-buffered like it, behind the output rings.
#define RCX_MC5_RING3_DW (2 * RCX_MC_CHUNK * RCX_LANES)
#define RCX_MC5_TREE_U4 (RCX_GROUPS * RCX_LANES) /* the model's groups; no staged divisors behind them (RCX_LDS_U4 has 64) */
#define RCX_MC5_LDS_U4 (RCX_MC_OUTPUT_DW / 4 + RCX_MC5_TREE_U4 + RCX_MC_RING_U4 + RCX_MC5_RING2_DW / 4 + RCX_MC5_RING3_DW / 4)

struct __attribute__((packed, aligned(4))) RcxU4Unaligned {
    u32 x, y, z, w;
};

// `extra` carries ran off the bytes the writer holds in registers: add them into the bytes already in the
// ring, newest first (cpprcoder.h:767-781).  Returns 1 if the carry wants to go below `safe_from`, where the
// bytes may have left for global memory already.  Rare (about 9e-5 per symbol on random data): out of line.
__device__ __attribute__((noinline, cold)) u32 rcx_stage_carry(u32* ring_lane, u32 pos, u32 safe_from, u32 extra)
{
    while (extra != 0 && pos > safe_from) {
        --pos;
        u32* w = ring_lane + ((pos >> 2) % RCX_OUT_RING_WORDS) * RCX_LANES;
        const u32 sh = 8u * (pos & 3u); // the ring holds memory-order dwords
        const u32 old = *w;
        const u32 v = ((old >> sh) & 0xFFu) + extra;
        *w = (old & ~(0xFFu << sh)) | ((v & 0xFFu) << sh);
        extra = v >> 8;
    }
    return extra != 0 && pos != 0 ? 1u : 0u; // (a carry out of the very first byte cannot happen: it starts as 0)
}

// A carry ran through all of the newest four bytes (StagedWriter::emit; `acc` has it already): it goes on in the ring, byte
// by byte.  First the two newest words go to their OWN slots as they were (the newest may so far only be in slot 64);
// everything older is in the ring already, and current: a byte stops changing, these paths apart, once it is no longer
// among the newest four.  Out of line: practically never on random data (tests/carry_runs.py builds the inputs).
__device__ __attribute__((noinline, cold)) u32 rcx_stage_far_carry(u32* ring_lane, u64 acc_after, u32 pos8, u32 safe_from, u32 far)
{
    if (!far) return 0;
    const u64 before = acc_after - 1;
    const u32 sh8 = (0u - pos8) & 24u;
    const u64 t = before << sh8;
    const u32 w = (pos8 - 8u) >> 5; // the word of the newest byte
    ring_lane[((w - 1u) % RCX_OUT_RING_WORDS) * RCX_LANES] = rcx_bswap((u32)(t >> 32));
    ring_lane[(w % RCX_OUT_RING_WORDS) * RCX_LANES] = rcx_bswap((u32)t);
    return rcx_stage_carry(ring_lane, pos8 >> 3, safe_from, 1u);
}

// The drain of a block's output ring (both multi-wave encoders): `piece` = the four ring words at `drained`, read earlier;
// it leaves if it lies below `lim`.  The predicated store is written out -- the compiler's version of
// `if (...) store` around three conditional pieces was forty instructions of execution-mask bookkeeping a chunk, on the
// wave that shares its SIMD with the arithmetic wave -- and a block that is more than one piece behind (a chunk makes 48
// bytes at most) goes out of line, where a loop may be a loop (in front of one the compiler waits for every store in flight).
__device__ __attribute__((noinline, cold)) u32 rcx_drain_more(const u32* ring_lane, u8* payload, u32 drained, u32 lim, bool live)
{
    while (__any(live && drained + 16 <= lim)) {
        if (live && drained + 16 <= lim) {
            const u32* w = ring_lane + ((drained >> 2) % RCX_OUT_RING_WORDS) * RCX_LANES; // (drained is a multiple of 16)
            RcxU4Unaligned piece;
            piece.x = w[0];
            piece.y = w[RCX_LANES];
            piece.z = w[2 * RCX_LANES];
            piece.w = w[3 * RCX_LANES];
            *reinterpret_cast<RcxU4Unaligned*>(payload + drained) = piece;
            drained += 16;
        }
    }
    return drained;
}
__device__ __forceinline__ u32 rcx_drain_piece(const u32* ring_lane, u8* payload, u32 drained, u32 lim, bool live, const RcxU4Unaligned& piece)
{
    const bool go = live && drained + 16 <= lim;
    {
        const u64 lanes = __ballot(go);
        u8* at = payload + drained;
        RcxV4 data;
        data.x = piece.x, data.y = piece.y, data.z = piece.z, data.w = piece.w;
        u64 saved;
        asm volatile("s_and_saveexec_b64 %[sv], %[go]\n\t"
                     "global_store_dwordx4 %[at], %[data], off\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [sv] "=&s"(saved)
                     : [go] "s"(lanes), [at] "v"(at), [data] "v"(data)
                     : "memory");
    }
    drained += go ? 16u : 0u;
    if (rcx_any(live && drained + 16 <= lim)) drained = rcx_drain_more(ring_lane, payload, drained, lim, live);
    return drained;
}

// The byte writer of the multi-wave encoders.  EncLane::emit gathers bytes in a register and lets four of them go when
// it holds five or more; that is a dozen selects a symbol.  Here the register is a WINDOW -- the newest eight bytes of
// the payload, newest lowest -- and the block's ring in LDS MIRRORS it: every symbol writes the two aligned words that hold
// the newest five to eight bytes (one ds_write2st64_b32: consecutive words of a block are 64 dwords apart), whether
// they are complete or not.  A carry (cpprcoder.h:767-781) is a 64-bit add on the window, made BEFORE the symbol's words
// are written, so whatever it changes among the newest four bytes is simply written again; only a carry that runs
// through all four of them -- the low half of the add overflows, which costs no instruction to notice -- has to go on
// in the ring itself (rcx_stage_carry; practically never on random data, adversarial inputs: tests/carry_runs.py).
// Ring slot 64 repeats slot 0 for the pair (63, 64): a word that lands there is the newest one, and it is written to
// its own slot as the older word of the next pair before anything reads it (the drain keeps RCX_OUT_MARGIN bytes back,
// finish() takes the newest word from the window).
struct StagedWriter {
    u64 acc;        // the newest 8 bytes of the payload as a number, newest byte lowest (before the stream: zeroes)
    // pos8 = 8 x the payload bytes produced so far (the reference's initial buffer_ = 0 is the first: EncLane), kept as the two
    // values a symbol needs of it, each moved by the symbol's k8 with one instruction (u32 arithmetic, wrap-around and all):
    u32 np;         // 0 - pos8: np & 24 is the shift that moves the window's end up to a word boundary
    u32 q;          // (pos8 - 40) << 3: q & RCX_OUT_SLOT_MASK is the byte offset of the older word's slot in the ring,
                    // ((pos - 1) / 4 - 1) mod 64 slots of 256 bytes (before the stream's fifth byte: slot 63, whose place is free)
    u32 pos;        // pos8 / 8 as of the last chunk_begins() / chunk_ends()
    u32 safe_from;  // bytes below this may have been drained (pos at the start of the chunk - RCX_OUT_MARGIN)
    u32 redo;
    u32* ring_lane; // word w of this block: ring_lane[(w % RCX_OUT_RING_WORDS) * RCX_LANES]; slot RCX_OUT_RING_WORDS: see above

    __device__ __forceinline__ void begin(u32* ring, u32* /*slot 64 follows the ring*/, u32 lane)
    {
        acc = 0;
        np = 0u - 8u;
        q = (8u - 40u) << 3;
        pos = 1;
        safe_from = 0;
        redo = 0;
        ring_lane = ring + lane;
    }
    __device__ __forceinline__ u32 pos8() const { return 0u - np; }
    // the lane's address in slot 0 as a number: a multiple of RCX_OUT_RING_BYTES + 4 x lane (McOutput), so a slot is ORed in
    __device__ __forceinline__ u32 slot0() const { return (u32)reinterpret_cast<uintptr_t>(ring_lane); }
    __device__ __forceinline__ void chunk_begins()
    {
        pos = pos8() >> 3;
        safe_from = pos > RCX_OUT_MARGIN ? pos - RCX_OUT_MARGIN : 0u;
    }
    __device__ __forceinline__ u32 chunk_ends()
    {
        pos = pos8() >> 3;
        return pos;
    }
    // the two aligned words that hold the newest 5..8 bytes, from the window
    __device__ __forceinline__ void mirror()
    {
        mirror_at(np & 24u, (q & RCX_OUT_SLOT_MASK) | slot0());
    }
    __device__ __forceinline__ void mirror_at(u32 sh8, u32 at_lds) // (an LDS address as a number: it passes through an asm statement)
    {
        const u64 t = acc << sh8;
        RcxLdsU32* at = reinterpret_cast<RcxLdsU32*>(at_lds);
        at[0] = rcx_bswap((u32)(t >> 32));
        at[RCX_LANES] = rcx_bswap((u32)t);
    }
    __device__ __forceinline__ void emit(u32 rec)
    {
        const u32 lo0 = (u32)acc;
        const u32 lo1 = lo0 + (rec & 1u);                  // cpprcoder.h:767-781
        const bool far = lo1 < lo0;                        // ... through all of the newest four bytes
        // (where the words go depends on the position alone: worked out between the two halves of the add, whose second
        // half may not follow the first at once.  The mask keeps the address inside the ring whatever q holds.)
        u32 sh8 = np & 24u;
        u32 at = (q & RCX_OUT_SLOT_MASK) | slot0();
        // (q passes through as well: seen through, the compiler keeps the sum of the k8 instead and pays an add a symbol for it)
        asm volatile("" : "+v"(sh8), "+v"(at), "+v"(q));
        acc = ((u64)((u32)(acc >> 32) + (far ? 1u : 0u)) << 32) | lo1;
        // (the far carry is looked at BEHIND the words' write: a branch on VCC directly behind the add that sets it held the
        // wave for 24 cycles a symbol.  rcx_stage_far_carry writes the two newest words itself, so the order does not matter
        // to what the ring holds afterwards.)
        mirror_at(sh8, at);
        if (rcx_any(far)) redo |= rcx_stage_far_carry(ring_lane, acc, pos8(), safe_from, far ? 1u : 0u);
        const u32 k8 = rec & 0x18u;
        acc = (acc << k8) | __builtin_amdgcn_ubfe(rec, 32u - k8, k8); // the k8 / 8 bytes that leave through the top of low
        np -= k8;
        q += k8 << 3; // (one v_lshl_add_u32)
    }
    // After the last symbol: the words below the newest one are in the ring (returns how many bytes that is); the newest
    // 1..4 bytes are handed over as EncLane's held bytes.
    __device__ __forceinline__ u32 finish(EncLane& enc)
    {
        mirror();
        pos = pos8() >> 3;
        const u32 flushed = ((pos - 1u) >> 2) << 2;
        enc.nacc8 = 8u * (pos - flushed);
        enc.acc = acc & ((1ull << enc.nacc8) - 1ull);
        enc.pos = flushed;
        return flushed;
    }
};

// ---------------------------------------------------------------------------
// What the multi-wave range encoders (rcx_enc_mc5_k, rcx_enc_static3_k) do alike behind their arithmetic wave: the
// writer wave, the drain of its rings and the closing stage.  Macros where the text sits inside the waves' loops, for
// RCX_ENTRY's reason (rcx_geom.hpp).
// ---------------------------------------------------------------------------
// The writer's side of a workgroup's LDS, dword arrays of one entry per lane.  BASE: the kernel's LDS array, aligned to
// RCX_OUT_RING_BYTES, + RCX_MC_OUTPUT_AT_DW (the ring comes first: StagedWriter ORs the slot into its address).
struct McOutput {
    u32* ring;      // RCX_OUT_RING_WORDS x 64: the writer's words on their way to global memory
    u32* dummy;     // (ring slot 64: repeats slot 0 for the writer's pair (63, 64))
    u32* final_low; // the arithmetic wave's last low, for the writer's finish()
    u32* pos;       // writer -> drain: bytes in the ring so far
    u32* drained;   // drain -> writer's finish: bytes stored so far
};
#define RCX_MC_OUTPUT(OUT, BASE)                                                                                       \
    McOutput OUT;                                                                                                      \
    OUT.ring = (BASE);                                                                                                 \
    OUT.dummy = OUT.ring + RCX_OUT_RING_WORDS * RCX_LANES;                                                             \
    OUT.final_low = OUT.dummy + RCX_LANES;                                                                             \
    OUT.pos = OUT.final_low + RCX_LANES;                                                                               \
    OUT.drained = OUT.pos + RCX_LANES

// The writer wave in pipeline step K: the records of chunk K-2 from RING2[(K-2)&1], in pairs (one ds_read2st64_b32);
// then its position to OUT_POS, for the drain of the next step.
#define RCX_MC_WRITER_STAGE(K, RING2, WR, OUT_POS)                                                                     \
    if ((K) >= 2) {                                                                                                    \
        const u32* rs2 = (RING2) + (((K)-2) & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;                                 \
        u32 ra_next = rs2[0], rb_next = rs2[RCX_LANES];                                                                \
        (WR).chunk_begins();                                                                                           \
        _Pragma("unroll") for (u32 s = 0; s < RCX_MC_CHUNK; s += 2)                                                    \
        {                                                                                                              \
            const u32 ra = ra_next, rb = rb_next;                                                                      \
            if (s + 2 < RCX_MC_CHUNK) ra_next = rs2[(s + 2) * RCX_LANES], rb_next = rs2[(s + 3) * RCX_LANES];          \
            (WR).emit(ra);                                                                                             \
            (WR).emit(rb);                                                                                             \
        }                                                                                                              \
        (OUT_POS)[lane] = (WR).chunk_ends();                                                                           \
    }

// The drain of a pipeline step, in two parts.  Asked for first: the writer's position (one barrier ago) and -- before it
// is known whether they may leave -- the next four words of the block's ring.  (Read and stored in one go, the five LDS
// reads' latency was the draining wave's: 28 cycles a symbol on the SIMD it shared with the arithmetic wave.)
#define RCX_MC_DRAIN_READ(P, PIECE, OUT_POS, WR, DRAINED)                                                              \
    {                                                                                                                  \
        P = (OUT_POS)[lane];                                                                                           \
        const u32* w = (WR).ring_lane + (((DRAINED) >> 2) % RCX_OUT_RING_WORDS) * RCX_LANES; /* (DRAINED is a multiple of 16: no wrap inside the piece) */ \
        PIECE.x = w[0];                                                                                                \
        PIECE.y = w[RCX_LANES];                                                                                        \
        PIECE.z = w[2 * RCX_LANES];                                                                                    \
        PIECE.w = w[3 * RCX_LANES];                                                                                    \
    }
// Stored later, behind the wave's other work: whole 16-byte pieces below (the writer's position - margin).  (Up to
// three pieces a chunk: 16 symbols make at most 48 bytes.  No loop: in front of a loop the compiler waits for every
// store in flight, and a store's round trip is a quarter of a chunk's time.)
#define RCX_MC_DRAIN_STORE(P, PIECE, WR, PAYLOAD, DRAINED, CAP, LIVE)                                                  \
    {                                                                                                                  \
        const u32 limit = (P) > RCX_OUT_MARGIN ? ((P)-RCX_OUT_MARGIN) & ~15u : 0u;                                     \
        DRAINED = rcx_drain_piece((WR).ring_lane, PAYLOAD, DRAINED, limit < (CAP) ? limit : (CAP), LIVE, PIECE);       \
    }

// The closing stage, behind the pipeline.  First the hand-over to the writer wave (role 1): the arithmetic wave's (role
// 0) last low and how far the drain wave got, whose pieces are in memory before the writer may read on behind them.
#define RCX_MC_CLOSE_HANDOVER(WAVE, DRAIN_WAVE, OUT, ENC, DRAINED)                                                     \
    if ((WAVE) == 0) OUT.final_low[lane] = (ENC).low;                                                                  \
    if ((WAVE) == (DRAIN_WAVE)) {                                                                                      \
        OUT.drained[lane] = DRAINED;                                                                                   \
        __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0) */                                                             \
    }                                                                                                                  \
    rcx_lds_barrier()
// Then the writer: what is still in the ring goes to PAYLOAD, the newest bytes and the last low to ENC for its finish()
// (cpprcoder.h:744-762, as in the one-wave coder).
#define RCX_MC_CLOSE_FLUSH(OUT, WR, ENC, PAYLOAD, CAP)                                                                 \
    {                                                                                                                  \
        u32 at_ = OUT.drained[lane];                                                                                   \
        const u32 flushed = (WR).finish(ENC);                                                                          \
        const u32 end = flushed < (CAP) ? flushed : (CAP);                                                             \
        for (; at_ < end; at_ += 4)                                                                                    \
            *reinterpret_cast<u32*>((PAYLOAD) + at_) = (WR).ring_lane[((at_ >> 2) % RCX_OUT_RING_WORDS) * RCX_LANES];  \
        (ENC).low = OUT.final_low[lane];                                                                               \
    }
// And the block's results: its size, an overflow of its slot, and its mark in REDO (a carry ran further back than the
// ring keeps bytes: the one-lane encoder codes the block again).
#define RCX_MC_CLOSE_REPORT(BYTES, ENC, WR, GEOM, BLK, SLOT, SIZES, STATUS, REDO)                                      \
    (SIZES)[BLK] = (ENC).overflow ? (u32)(SLOT) : (BYTES);                                                             \
    if ((ENC).overflow) rcx_flag(STATUS, RCX_ST_CAPACITY, rcx_id(GEOM, BLK));                                          \
    (REDO)[BLK] = ((WR).redo != 0 && !(ENC).overflow) ? 1u : 0u

template <bool FULL>
__device__ __forceinline__ void rcx_mc5_pipeline(u32 wave, u32 lane, u32 len, u32 nchunks, const u8* in,
                                                 const u32* __restrict__ divq, const Tree& tree,
                                                 u32* ring, u32* ring2, u32* ring3, EncLane& enc, StagedWriter& wr,
                                                 u32* out_pos, u32& drained, u8* payload, u32 cap, bool live)
{
    // wave roles: 0 arithmetic, 1 writer, 2 model level 2, 3 model leaf level, 4 model level 1, 5 drain, 6 model level 3
    // (a pipeline step ends at the workgroup's barrier, in whichever of the two loops below a wave runs)
#if defined(RCX_STAMP)
    unsigned long long stamp_wait_ = 0;
    const unsigned long long stamp_begin_ = __builtin_amdgcn_s_memtime();
#define RCX_MC5_STEP_ENDS()                                                \
    {                                                                      \
        const unsigned long long t0_ = __builtin_amdgcn_s_memtime();       \
        rcx_lds_barrier();                                                 \
        stamp_wait_ += __builtin_amdgcn_s_memtime() - t0_;                 \
    }
#define RCX_MC5_STAMPS_OUT()                                               \
    if (blockIdx.x == 7 && lane == 0) {                                    \
        rcx_stamp_out[wave * 2] = __builtin_amdgcn_s_memtime() - stamp_begin_; \
        rcx_stamp_out[wave * 2 + 1] = stamp_wait_;                         \
    }
#else
#define RCX_MC5_STEP_ENDS() rcx_lds_barrier()
#define RCX_MC5_STAMPS_OUT()
#endif
    // Two waves of a SIMD share its issue slots by priority, then age.  The level-1 wave is the younger one beside the
    // arithmetic wave and was the kernel's pole (busy 174 of 177 cycles a symbol); the arithmetic wave has 45 to give.
    // (Measured on full 64 KiB blocks, 64 to a workgroup; set for the guarded pipeline and single streams as well, where
    // its effect is not measured.  It changes the order in which instructions issue, never a result.)
    if ((RCX_MC5_PRIO >> wave) & 1u) __builtin_amdgcn_s_setprio(1);
    // The arithmetic wave's divisors, in registers as the quad decoder has them (rcx_quad.hpp, RCX_QUAD_DIVQ_DW): the 16
    // multipliers and 16 increments of a chunk are eight 16-byte registers that every lane loads alike, each loaded again
    // -- with the next chunk's quarter -- right behind its quarter's last symbol, and waited for once, at the top of the
    // next chunk (the wave has no other global traffic, and a barrier lies in between).  Vector loads through a zero the
    // compiler cannot see through: scalar ones would share lgkmcnt with the wave's LDS reads.  A short block's last chunk
    // loads the group behind it: the table has 2 * RCX_STAGE spare entries (rcx_ctx.hpp ensure_divtab).
    // The wave has a loop of its own, so that these 32 registers are not carried through the other waves' steps (carried
    // through, they are split around the model waves' 64 registers of groups, and the chain waits for the copies).
    if (wave == 0) {
        U4 dm[4], di[4];
        u32 prev_k8 = 0; // the renormalising shift of the symbol before (EncLane::arith_i)
        u32 vz;
        asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
        const u32* dq = divq + vz;
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
            dm[q] = reinterpret_cast<const U4*>(dq)[q];
            di[q] = reinterpret_cast<const U4*>(dq + 16)[q];
        }
        RCX_MC5_STEP_ENDS(); // (step 0: the model waves' first chunk)
        for (u32 k = 1; k <= nchunks; ++k) {
            // ---- arithmetic: chunk k-1, records into ring2[(k-1)&1] ----
            {
                const u32 i0 = (k - 1) * RCX_MC_CHUNK;
                // the chunk's divisors: asked for a chunk ago, waited for here, once, by a statement that reads them
                asm volatile("" ::"v"(dm[0].x), "v"(di[0].x), "v"(dm[1].x), "v"(di[1].x), "v"(dm[2].x), "v"(di[2].x), "v"(dm[3].x), "v"(di[3].x));
                // their shift: floor(log2(total)) is one value for the chunk's 16 totals (the powers of two from 256 up are
                // multiples of 16); wave-uniform, a scalar
                const u32 sh = 31u - rcx_clz(256u + i0);
                const u32* dq_next = dq + (size_t)k * RCX_QUAD_DIVQ_DW; // chunk k - 1 is group k - 1 of the table
                // the model waves' answers: field f of symbol s of lane l at dword RCX_RING_AT(s, f) + RCX_RING_LANE * l
                const u32* rs = ring + ((k - 1) & 1u) * (4 * RCX_MC_CHUNK * RCX_LANES) + RCX_RING_LANE * lane;
                const u32* rs3 = ring3 + ((k - 1) & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane; // (level 3: two symbols per ds_read2st64_b32)
                u32* ws2 = ring2 + ((k - 1) & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;
                U4 eq[RCX_MC_CHUNK];
                u32 c3q[RCX_MC_CHUNK];
                u32 rec_even = 0;
#define RCX_A_U4_AT(V, C) ((C) == 0 ? (V).x : (C) == 1 ? (V).y : (C) == 2 ? (V).z : (V).w)
#define RCX_A_ISSUE(T)                                                                                              \
    {                                                                                                               \
        eq[T].x = rs[RCX_RING_AT((T), 0)], eq[T].y = rs[RCX_RING_AT((T), 1)], eq[T].z = rs[RCX_RING_AT((T), 2)];    \
        eq[T].w = rs[RCX_RING_AT((T), 3)];                                                                          \
        if (((T)&1u) == 0) c3q[T] = rs3[(T)*RCX_LANES], c3q[(T) + 1] = rs3[((T) + 1) * RCX_LANES];                   \
    }
#pragma unroll
                for (u32 t = 0; t < RCX_ARITH_AHEAD; ++t) RCX_A_ISSUE(t);
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    if (s + RCX_ARITH_AHEAD < RCX_MC_CHUNK) RCX_A_ISSUE(s + RCX_ARITH_AHEAD);
                    const U4 e = eq[s];
                    u32 rec = 0; // past the end of a short block: a record that does nothing
                    if (FULL || i0 + s < len)
                        rec = enc.arith_i(e.x + e.y + e.z + c3q[s], e.w, RCX_A_U4_AT(dm[s >> 2], s & 3u), RCX_A_U4_AT(di[s >> 2], s & 3u), sh, prev_k8);
                    if ((s & 3u) == 3u) { // the quarter's registers are free: the next chunk's quarter
                        // (held in place by statements that no memory access is moved across: left to the compiler, all eight
                        // loads gather behind the first quarter, in other registers)
                        asm volatile("" ::: "memory");
                        dm[s >> 2] = reinterpret_cast<const U4*>(dq_next)[s >> 2];
                        di[s >> 2] = reinterpret_cast<const U4*>(dq_next + 16)[s >> 2];
                        asm volatile("" ::: "memory");
                    }
                    // two symbols' records leave as one ds_write2st64_b32 (consecutive symbols are 64 dwords apart): an LDS
                    // instruction costs a lone wave 12-16 cycles of issue whatever it carries (tools/diag/ubench.hip k_t_*)
                    if ((s & 1u) == 0) rec_even = rec;
                    else {
                        ws2[(s - 1) * RCX_LANES] = rec_even;
                        ws2[s * RCX_LANES] = rec;
                    }
                }
#undef RCX_A_ISSUE
#undef RCX_A_U4_AT
            }
            RCX_MC5_STEP_ENDS();
        }
        RCX_MC5_STEP_ENDS(); // (step nchunks + 1: the writer's last chunk)
        RCX_MC5_STAMPS_OUT();
        return;
    }
    U4 piece_ahead;
    piece_ahead.x = piece_ahead.y = piece_ahead.z = piece_ahead.w = 0;
    if (FULL && wave >= 2 && wave != RCX_DRAIN_WAVE && nchunks > 0) piece_ahead = *reinterpret_cast<const U4*>(in);
    u32 l3a = 64, l3b = 128, l3c = 192; // level-3 wave: its sums (cpprcoder.h:1094-1132: every count 1)
    for (u32 k = 0; k <= nchunks + 1; ++k) {
        if (wave == 1) {
            RCX_MC_WRITER_STAGE(k, ring2, wr, out_pos) // chunk k-2
        } else if (wave == RCX_DRAIN_WAVE) {
            // ---- drain: what the writer had a barrier ago ----
            u32 drain_p;
            RcxU4Unaligned drain_piece;
            RCX_MC_DRAIN_READ(drain_p, drain_piece, out_pos, wr, drained)
            RCX_MC_DRAIN_STORE(drain_p, drain_piece, wr, payload, drained, cap, live)
        } else if (k < nchunks) {
            // ---- model: chunk k ----
            const u32 i0 = k * RCX_MC_CHUNK;
            u32* ws = ring + (k & 1u) * (4 * RCX_MC_CHUNK * RCX_LANES) + RCX_RING_LANE * lane;
            U4 piece;
            if (FULL) {
                piece = piece_ahead;
                if (k + 1 < nchunks) piece_ahead = *reinterpret_cast<const U4*>(in + i0 + RCX_MC_CHUNK);
            } else if (i0 + RCX_MC_CHUNK <= len && (reinterpret_cast<uintptr_t>(in) & 15u) == 0) {
                piece = *reinterpret_cast<const U4*>(in + i0); // a whole, aligned chunk of a ragged block (or of a single stream)
            } else {
                u32 w[4] = {0, 0, 0, 0};
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s)
                    if (i0 + s < len) w[s >> 2] |= (u32)in[i0 + s] << (8 * (s & 3));
                piece.x = w[0];
                piece.y = w[1];
                piece.z = w[2];
                piece.w = w[3];
            }
            // Software pipeline, RCX_MODEL_AHEAD symbols deep: the group reads AND the ds_add updates of symbol
            // s + AHEAD are issued before the sums of symbol s are formed.  LDS executes a wave's operations in order,
            // so the reads of a later symbol still see the updates of the earlier ones, and their latency -- 60 cycles
            // and more with five waves on the LDS unit, i.e. more than one symbol of a light wave -- hides behind the
            // arithmetic of the symbols in between (the updates need only the symbol, not the read data).
            U4 ga[RCX_MC_CHUNK], gb[RCX_MC_CHUNK]; // (indices are compile-time constants: registers)
            u32 held = 0, held_f = 0;
            if (wave == 2) {
#define RCX_M2_ISSUE(T)                                                       \
    {                                                                         \
        const u32 c_ = rcx_byte_of(piece, (T));                               \
        gb[T] = tree.group(RCX_G_L2 + (c_ >> 6));                             \
        if (FULL || i0 + (T) < len) tree.bump(RCX_G_L2 + (c_ >> 6), (c_ >> 4) & 3); \
    }
#pragma unroll
                for (u32 t = 0; t < RCX_MODEL_AHEAD; ++t) RCX_M2_ISSUE(t);
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    if (s + RCX_MODEL_AHEAD < RCX_MC_CHUNK) RCX_M2_ISSUE(s + RCX_MODEL_AHEAD);
                    const u32 cc = rcx_byte_of(piece, s);
                    const u32 sum32 = rcx_pre4(gb[s], (cc >> 4) & 3);
                    if (FULL) { // (pairs: one ds_write2st64_b32)
                        if ((s & 1u) == 0) held = sum32;
                        else ws[RCX_RING_AT(s - 1, 0)] = held, ws[RCX_RING_AT(s, 0)] = sum32;
                    } else if (i0 + s < len) ws[RCX_RING_AT(s, 0)] = sum32;
                }
#undef RCX_M2_ISSUE
            } else if (wave == 4) {
#define RCX_M1_ISSUE(T)                                                       \
    {                                                                         \
        const u32 c_ = rcx_byte_of(piece, (T));                               \
        ga[T] = tree.group(RCX_G_L1 + (c_ >> 4));                             \
        if (FULL || i0 + (T) < len) tree.bump(RCX_G_L1 + (c_ >> 4), (c_ >> 2) & 3); \
    }
#pragma unroll
                for (u32 t = 0; t < RCX_MODEL_AHEAD; ++t) RCX_M1_ISSUE(t);
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    if (s + RCX_MODEL_AHEAD < RCX_MC_CHUNK) RCX_M1_ISSUE(s + RCX_MODEL_AHEAD);
                    const u32 cc = rcx_byte_of(piece, s);
                    const u32 sum1 = rcx_pre4(ga[s], (cc >> 2) & 3);
                    if (FULL) { // (pairs: one ds_write2st64_b32)
                        if ((s & 1u) == 0) held = sum1;
                        else ws[RCX_RING_AT(s - 1, 1)] = held, ws[RCX_RING_AT(s, 1)] = sum1;
                    } else if (i0 + s < len) ws[RCX_RING_AT(s, 1)] = sum1;
                }
#undef RCX_M1_ISSUE
            } else if (wave == RCX_L3_WAVE) {
                // Level 3 -- one group per block -- lives in registers as three prefix sums (symbols below 64, 128, 192 so
                // far): three compares serve both the select and the update.  No LDS access but the hand-over, and no test
                // for the end of a short block: what follows a block's last symbol is never read.
                u32* ws3 = ring3 + (k & 1u) * (RCX_MC_CHUNK * RCX_LANES) + lane;
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    const u32 cc = rcx_byte_of(piece, s);
                    u32 cum3;
                    u64 m1_, m2_, m3_, cz_;
                    asm volatile("v_cmp_gt_u32_e64 %[m3], %[k192], %[c]\n\t" /* (no literals in this encoding: 192, 128 from registers) */
                                 "v_cmp_gt_u32_e64 %[m2], %[k128], %[c]\n\t"
                                 "v_cmp_gt_u32_e64 %[m1], 64, %[c]\n\t"
                                 "v_cndmask_b32_e64 %[x], %[pc], %[pb], %[m3]\n\t"
                                 "v_cndmask_b32_e64 %[x], %[x], %[pa], %[m2]\n\t"
                                 "v_cndmask_b32_e64 %[x], %[x], 0, %[m1]\n\t"
                                 "v_addc_co_u32_e64 %[pc], %[cz], %[pc], 0, %[m3]\n\t"
                                 "v_addc_co_u32_e64 %[pb], %[cz], %[pb], 0, %[m2]\n\t"
                                 "v_addc_co_u32_e64 %[pa], %[cz], %[pa], 0, %[m1]"
                                 : [x] "=&v"(cum3), [pa] "+v"(l3a), [pb] "+v"(l3b), [pc] "+v"(l3c), [m1] "=&s"(m1_), [m2] "=&s"(m2_),
                                   [m3] "=&s"(m3_), [cz] "=&s"(cz_)
                                 : [c] "v"(cc), [k192] "s"(192u), [k128] "s"(128u));
                    if ((s & 1u) == 0) held = cum3; // (pairs: one ds_write2st64_b32)
                    else ws3[(s - 1) * RCX_LANES] = held, ws3[s * RCX_LANES] = cum3;
                }
            } else {
                // The symbol's count is READ (a ds_read_b32 at the address the bump computes anyway), directly in front of its own
                // bump: LDS serves a wave's operations in order, so it holds every earlier symbol's bump and not its own.  From
                // the group it is (sum of the first p + 1) - (sum of the first p), four instructions more (rcx_pre4_sel4).  Past
                // a short block's end the read runs on, as the group read does; its value is not used there.
                u32 fq[RCX_MC_CHUNK];
#define RCX_M0_ISSUE(T)                                                       \
    {                                                                         \
        const u32 c_ = rcx_byte_of(piece, (T));                               \
        ga[T] = tree.group(RCX_G_L0 + (c_ >> 2));                             \
        fq[T] = *tree.at(RCX_G_L0 + (c_ >> 2), c_ & 3);                       \
        if (FULL || i0 + (T) < len) tree.bump(RCX_G_L0 + (c_ >> 2), c_ & 3);  \
    }
#pragma unroll
                for (u32 t = 0; t < RCX_MODEL_AHEAD; ++t) RCX_M0_ISSUE(t);
#pragma unroll
                for (u32 s = 0; s < RCX_MC_CHUNK; ++s) {
                    if (s + RCX_MODEL_AHEAD < RCX_MC_CHUNK) RCX_M0_ISSUE(s + RCX_MODEL_AHEAD);
                    const u32 cc = rcx_byte_of(piece, s);
                    const u32 sum0 = rcx_pre4(ga[s], cc & 3), f0 = fq[s];
                    if (FULL) { // (pairs: fields 2 and 3 are one aligned qword, and the compiler makes the four stores ONE ds_write2st64_b64)
                        if ((s & 1u) == 0) held = sum0, held_f = f0;
                        else {
                            ws[RCX_RING_AT(s - 1, 2)] = held, ws[RCX_RING_AT(s, 2)] = sum0;
                            ws[RCX_RING_AT(s - 1, 3)] = held_f, ws[RCX_RING_AT(s, 3)] = f0;
                        }
                    } else if (i0 + s < len) {
                        ws[RCX_RING_AT(s, 2)] = sum0;
                        ws[RCX_RING_AT(s, 3)] = f0;
                    }
                }
#undef RCX_M0_ISSUE
            }
        }
        RCX_MC5_STEP_ENDS();
    }
    RCX_MC5_STAMPS_OUT();
#undef RCX_MC5_STEP_ENDS
#undef RCX_MC5_STAMPS_OUT
}

template <class G = RcxBlocks>
__global__ __launch_bounds__(RCX_MC5_THREADS) void rcx_enc_mc5_k(const u8* __restrict__ src, u64 n, u32 block, u64 nblocks,
                                                                u8* __restrict__ slots, u64 slot, u32* __restrict__ sizes,
                                                                const u32* __restrict__ divq, u32* status,
                                                                u32* __restrict__ redo, u32 lanes_used, const G g = G())
{
    __shared__ __attribute__((aligned(RCX_OUT_RING_BYTES))) U4 lds[RCX_MC5_LDS_U4]; // (McOutput first: RCX_MC_OUTPUT)
    static_assert(__alignof__(lds) % RCX_OUT_RING_BYTES == 0 && RCX_MC5_LDS_U4 * 16 <= 160 * 1024, "the output ring's place in LDS");
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = RCX_MC5_ROLE(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)); // the wave's ROLE (see RCX_MC5_ROLE)
    // lanes_used (1..64) of the 64 lanes carry a block; the others idle along (rcx_api.hip picks it from the
    // block count so that every CU has a workgroup before any workgroup carries 64 blocks)
    const bool in_use = lane < lanes_used;
    const u64 blk = in_use ? (u64)blockIdx.x * lanes_used + lane : nblocks;
    RCX_ENTRY(g, blk, nblocks, n, block);
    RCX_ENTRY_SLOTS(g, blk, slots, slot);

    RCX_MC_OUTPUT(oq, reinterpret_cast<u32*>(lds) + RCX_MC_OUTPUT_AT_DW);
    U4* behind = lds + (RCX_MC_OUTPUT_AT_DW + RCX_MC_OUTPUT_DW) / 4;
    Tree tree{reinterpret_cast<u32*>(behind) + (RCX_TREE_PLANAR ? 1 : 4) * lane};
    u32* ring = reinterpret_cast<u32*>(behind + RCX_MC5_TREE_U4); // (no divisor staging behind the tree: rcx_mc5_pipeline)
    u32* ring2 = reinterpret_cast<u32*>(behind + RCX_MC5_TREE_U4 + RCX_MC_RING_U4);
    u32* ring3 = ring2 + RCX_MC5_RING2_DW;

    const u32 maxlen = rcx_wave_max(len);
    bool full;
    if constexpr (G::items) {
        // Not RCX_ALL_FULL, which is never true with items: this kernel has the FULL pipeline for them as well
        // (16-byte loads, no per-symbol length test), where every entry of the workgroup has the
        // same length, a multiple of 16, at an aligned address -- a batch of equal items is then coded as its blocks
        // would be.  (A lane without an entry reads the launch's first entry along, which is at least as long: rcx_where.)
        full = __all((!in_use || (live && len == maxlen)) && ((reinterpret_cast<uintptr_t>(src) + at) & 15u) == 0) && (maxlen % 16u == 0);
    } else {
        // (RCX_ALL_FULL, but for the lanes that carry no block: they do not count)
        full = __all(!in_use || (live && len == block)) && (block % 16u == 0) && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0);
    }
    const u8* in = src + at; // (a lane without a block reads the first block along)
    const u32 nchunks = (maxlen + RCX_MC_CHUNK - 1) / RCX_MC_CHUNK;

    EncLane enc;
    u8* wave_slots = slots + (u64)blockIdx.x * lanes_used * slot;
    enc.idle(wave_slots); // wave 0 uses low/range; wave 1 takes over for finish()
    StagedWriter wr;
    wr.begin(oq.ring, oq.dummy, lane);
    u32 drained = 0;
    U4 v;
    if (wave == 1) {
        if (live) enc.begin(wave_slots, lane * (u32)slot, (u32)slot, len);
        oq.pos[lane] = 0;
    } else if (wave == 2) { // cpprcoder.h:1094-1132: every count 1 (level 3: registers of rcx_mc5_pipeline)
        v.x = v.y = v.z = v.w = 16;
        for (u32 g = RCX_G_L2; g < RCX_G_L1; ++g) tree.store(g, v);
    } else if (wave == 4) {
        v.x = v.y = v.z = v.w = 4;
        for (u32 g = RCX_G_L1; g < RCX_G_L0; ++g) tree.store(g, v);
    } else if (wave == 3) {
        v.x = v.y = v.z = v.w = 1;
        for (u32 g = RCX_G_L0; g < RCX_GROUPS; ++g) tree.store(g, v);
    }
    rcx_lds_barrier();

    u8* payload = wave_slots + (u64)lane * slot + 4;
    const u32 cap = ((u32)slot - 4) & ~3u; // as EncLane::begin
    if (full) rcx_mc5_pipeline<true>(wave, lane, len, nchunks, in, divq, tree, ring, ring2, ring3, enc, wr, oq.pos, drained, payload, cap, live);
    else rcx_mc5_pipeline<false>(wave, lane, len, nchunks, in, divq, tree, ring, ring2, ring3, enc, wr, oq.pos, drained, payload, cap, live);

    RCX_MC_CLOSE_HANDOVER(wave, RCX_DRAIN_WAVE, oq, enc, drained);
    if (wave == 1 && live) {
        RCX_MC_CLOSE_FLUSH(oq, wr, enc, payload, cap)
        const u32 bytes = enc.finish();
        RCX_MC_CLOSE_REPORT(bytes, enc, wr, g, blk, slot, sizes, status, redo);
    } else if (wave == 1 && blk < nblocks) {
        redo[blk] = 0;
    }
}
