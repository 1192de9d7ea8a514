// rcx_streams.hpp -- single streams with the reference's sink semantics (one block, lane 0 of one wave), whole
// (rcx_stream_encode / rcx_stream_decode) and fed piece by piece (rcx_dstream, rcx_estream).
//
// The whole-stream calls launch by themselves, not through the launch tables (rcx_launch.hpp): one block, on lengths below
// RCX_MIN_BLOCK and above RCX_MAX_BLOCK too, and with the instantiations that track where a sink filled or the input ran dry.
#pragma once
#include "rcx_launch.hpp"

#define RCX_DSTREAM_CHUNK (1u << 20) /* symbols per launch */

// The resumable single-stream decoder: AdaptiveRangeDecoder<T>::decode fed piece by piece (cpprcoder.h:872-924).
struct rcx_dstream {
    rcx_ctx* ctx = nullptr;
    DevBuf<RcxDState> state;
    DevBuf<u8> in;              // the bytes accepted so far that the decoder has not read yet (+ what it read since the last growth)
    u64 in_base = 0;            // where in the stream in[0] is
    u64 in_bytes = 0;
    u64 consumed = 0;           // how far the decoder has read (RcxDState::consumed)
    DevBuf<u8> out;             // one launch's symbols
    DevBuf<u32> result;         // {made, finished, declared, produced, consumed lo, consumed hi}
    PinBuf<u32> result_host;
    bool finished = false;
    u32 declared = 0, produced = 0;
};

// The resumable single-stream encoder: AdaptiveRangeEncoder<T>::encode fed piece by piece (cpprcoder.h:697-720).
struct rcx_estream {
    rcx_ctx* ctx = nullptr;
    DevBuf<RcxEState> state;
    DevBuf<RcxEState> backup;     // the state before the last call (rcx_estream_rewind)
    DevBuf<u8> slot;              // the stream so far (slot_bytes of it, and 64 to spare)
    u64 slot_bytes = 0;
    DevBuf<u8> tail_backup;       // the bytes of `slot` the last call could change
    u64 tail_from = 0, tail_bytes = 0;
    DevBuf<u8> in;                // the piece being fed
    DevBuf<u32> result;
    PinBuf<u32> result_host;
    u32 declared = 0, consumed = 0;
    u64 written = 0;              // payload bytes handed on so far (the reference's writeByte count)
    u32 backup_consumed = 0;
    u64 backup_written = 0;
    bool have_backup = false, dead = false, finished = false;
    u64 pos_hint = 0;             // payload bytes in memory after the last call (how far a call can have changed things)
};

namespace
{

u32 le32(const uint8_t* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

// What rcx_stream_encode codes: the source's `n` bytes in h_in.
int stage_source(rcx_ctx* c, const uint8_t* src, u32 n)
{
    const int r = c->h_in.reserve((u64)n + 64);
    if (r != RCX_OK) return r;
    if (n) HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    return RCX_OK;
}

// What rcx_stream_decode decodes: the stream in h_in, its table {0, comp_size} in h_off, room for `out` symbols in h_out.
int stage_stream(rcx_ctx* c, const uint8_t* comp, u64 comp_size, u64 out)
{
    const int r = reserve_staging(c, comp_size, out, 2);
    if (r != RCX_OK) return r;
    const u64 offs[2] = {0, comp_size};
    HIP_TRY(hipMemcpy(c->h_in, comp, comp_size, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_off, offs, sizeof(offs), hipMemcpyHostToDevice));
    return RCX_OK;
}

// rcx_stream_encode's end where the reference hands back a bool (the static coder, rANS): the latch, then the whole
// stream, which begins *d_start bytes into the slot (rANS: the encoders write backwards) or with it (nullptr).
int fetch_stream(rcx_ctx* c, const u32* d_start, uint8_t* dst, u64 dst_cap, u64 sink_capacity, uint64_t* dst_size)
{
    HIP_TRY(hipGetLastError());
    const int r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (r != RCX_OK) return r;
    u32 size = 0, start = 0;
    HIP_TRY(hipMemcpy(&size, c->sizes, sizeof(u32), hipMemcpyDeviceToHost));
    if (d_start) HIP_TRY(hipMemcpy(&start, d_start, sizeof(u32), hipMemcpyDeviceToHost));
    *dst_size = size;
    if (size > sink_capacity || size > dst_cap) return RCX_E_CAPACITY;
    HIP_TRY(hipMemcpy(dst, c->slots + start, size, hipMemcpyDeviceToHost));
    return RCX_OK;
}

// The whole stream is wanted and the sink has room: a 4-lane decoder (`launch_fast`) runs the chain about three times as
// fast as a lone lane.  It only knows complete, valid streams; anything else (input that runs dry: Pending,
// cpprcoder.h:901-903; a target past the table) it reports -- the latch, its mark in redo[0] -- and *done stays false:
// the caller's exact one-lane kernel decodes the stream again.
template <class Launch>
int decode_fast(rcx_ctx* c, Launch launch_fast, uint8_t* dst, u64 count, uint64_t* dst_size, bool* done)
{
    const int r = ensure_redo(c, 1);
    if (r != RCX_OK) return r;
    launch_fast();
    HIP_TRY(hipGetLastError());
    u32 marked = 0;
    const int fast = rcx_ctx_sync_status(c, nullptr, nullptr); // (clears the latch)
    HIP_TRY(hipMemcpy(&marked, c->redo, sizeof(u32), hipMemcpyDeviceToHost));
    if (fast != RCX_OK || marked != 0) return RCX_OK;
    HIP_TRY(hipMemcpy(dst, c->h_out, count, hipMemcpyDeviceToHost));
    *dst_size = count;
    *done = true;
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_stream_encode(rcx_ctx* c, int coder, const uint8_t* src, uint32_t n,
                      uint8_t* dst, uint64_t dst_cap, uint64_t sink_capacity, uint64_t* dst_size, uint32_t* request_size)
{
    if (!c || !dst || !dst_size || (n && !src)) return RCX_E_ARG;
    if (!coder_ok(coder) || n > RCX_MAX_STREAM) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    if (request_size) *request_size = 0;
    const u32 block = n < RCX_MIN_BLOCK ? RCX_MIN_BLOCK : n;
    if (is_rans(coder)) {
        // rANS::encode / encode_simd (cppans.h:497-530, :567-607): one block; RCX_ERROR where the reference returns 0
        // (it asserts 0 < src_size; its destination cannot be larger than u32 either)
        if (n == 0 || n > RCX_MAX_RANS_STREAM) return RCX_ERROR;
        int rr = reserve(c, block, block, coder);
        if (rr == RCX_OK) rr = stage_source(c, src, n);
        if (rr != RCX_OK) return rr;
        const u64 rslot = rcx_block_bound_for(coder, block);
        if (coder == RCX_CODER_RANS8)
            hipLaunchKernelGGL(rcx_enc_rans_k<true>, dim3(1), dim3(256), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, rslot, c->sizes,
                               c->starts, c->status);
        else
            hipLaunchKernelGGL(rcx_enc_rans_k<false>, dim3(1), dim3(256), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, rslot, c->sizes,
                               c->starts, c->status);
        return fetch_stream(c, c->starts, dst, dst_cap, sink_capacity, dst_size);
    }
    const bool longer = n > RCX_MAX_BLOCK; // past the table halving of cpprcoder.h:1138: the lane divides by its own total
    const u64 slot = rcx_block_bound(block);
    int r = longer ? RCX_OK : ensure_divtab(c, block);
    if (r == RCX_OK) r = c->slots.reserve(slot + 256);
    if (r == RCX_OK) r = c->sizes.reserve(2);
    if (r == RCX_OK) r = stage_source(c, src, n);
    if (r != RCX_OK) return r;
    // The one-wave kernels on the one block: the whole coding (redo = nullptr), or the pass behind a multi-wave kernel
    // that takes over if a carry outran that one's rings (see encode_launches).
    auto adaptive_pass = [&](const u32* redo) {
        hipLaunchKernelGGL((rcx_enc_adaptive_k<false, false>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot,
                           c->sizes, c->divtab(), c->status, 0u, static_cast<u32*>(nullptr), redo);
    };
    auto static_pass = [&](const u32* redo) {
        hipLaunchKernelGGL(rcx_enc_static_k, dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot, c->sizes, c->status, redo);
    };
    if (coder == RCX_CODER_STATIC) {
        // RangeEncoder<T>::encode (cpprcoder.h:375-458) returns a bool; the caller (the facade) replays the
        // sink calls itself, so the whole stream is handed back: RCX_OK, or RCX_E_CAPACITY if dst is too small.
        if (c->enc_variant >= 2 && n >= RCX_MIN_BLOCK && n <= RCX_MAX_BLOCK) {
            // one chain runs faster through the three-wave encoder (table lookups / arithmetic / writer on three SIMDs)
            // than on a lone lane
            if ((r = ensure_redo(c, 1)) != RCX_OK) return r;
            hipLaunchKernelGGL(rcx_enc_static3_k, dim3(1), dim3(RCX_ST3_THREADS), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot,
                               c->sizes, c->status, c->redo, 1u);
            static_pass(c->redo);
        } else {
            static_pass(nullptr);
        }
        return fetch_stream(c, nullptr, dst, dst_cap, sink_capacity, dst_size);
    }
    if (longer) {
        hipLaunchKernelGGL((rcx_enc_adaptive_k<false, true>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot,
                           c->sizes, c->divtab(), c->status, 0u, static_cast<u32*>(nullptr), static_cast<const u32*>(nullptr));
    } else if (c->enc_variant == 3 && n >= RCX_MIN_BLOCK) {
        // One stream is one chain, and the five-wave encoder runs a chain about four times as fast as a lone lane does
        // (its model, arithmetic and writer are five instruction streams on four SIMDs): one block, one lane in use.
        if ((r = ensure_redo(c, 1)) != RCX_OK) return r;
        hipLaunchKernelGGL(rcx_enc_mc5_k, dim3(1), dim3(RCX_MC5_THREADS), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot, c->sizes,
                           c->divq(), c->status, c->redo, 1u);
        adaptive_pass(c->redo);
    } else {
        adaptive_pass(nullptr);
    }
    HIP_TRY(hipGetLastError());
    r = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (r != RCX_OK) return r;
    u32 size = 0;
    HIP_TRY(hipMemcpy(&size, c->sizes, sizeof(u32), hipMemcpyDeviceToHost));
    const u64 cap16 = sink_capacity < 4 ? 4 : sink_capacity; // the header went through the growing write()
    if ((u64)size - 4 <= cap16) { // every writeByte fits; the final write(4) grows the sink (cpprcoder.h:1031-1045)
        *dst_size = size;
        if (size > dst_cap) return RCX_E_CAPACITY;
        HIP_TRY(hipMemcpy(dst, c->slots, size, hipMemcpyDeviceToHost));
        return RCX_OK;
    }
    // The sink fills.  Second pass: replay the reference's delayed writer to find the symbol.
    *dst_size = cap16;
    if (cap16 > dst_cap) return RCX_E_CAPACITY;
    if (longer)
        hipLaunchKernelGGL((rcx_enc_adaptive_k<true, true>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot,
                           c->sizes, c->divtab(), c->status, (u32)(cap16 - 4), c->status + 2, static_cast<const u32*>(nullptr));
    else
        hipLaunchKernelGGL((rcx_enc_adaptive_k<true, false>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)n, block, (u64)1, c->slots, slot,
                           c->sizes, c->divtab(), c->status, (u32)(cap16 - 4), c->status + 2, static_cast<const u32*>(nullptr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(c->status_host, c->status, 4 * sizeof(u32), hipMemcpyDeviceToHost));
    const u32 fail_at = c->status_host[2];
    HIP_TRY(hipMemcpy(dst, c->slots, cap16, hipMemcpyDeviceToHost)); // what was written before the sink filled
    if (fail_at != 0xFFFFFFFFu) { // cpprcoder.h:708-711
        if (request_size) *request_size = n - fail_at;
        return RCX_PENDING;
    }
    return RCX_OK; // only finish() failed and encode() ignores that (cpprcoder.h:716)
}

int rcx_stream_decode(rcx_ctx* c, int coder, const uint8_t* comp, uint64_t comp_size,
                      uint8_t* dst, uint64_t sink_capacity, uint64_t* dst_size, uint32_t* request_size)
{
    if (!c || !dst || !dst_size || (comp_size && !comp)) return RCX_E_ARG;
    if (!coder_ok(coder) || comp_size > 0xFFFFFFFFull) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    if (request_size) *request_size = 0;
    if (is_rans(coder)) {
        // rANS::decode / decode_simd (cppans.h:532-564, :609-649): RCX_ERROR where the reference returns 0 (or would
        // leave its arrays: a header that is not a scaled cumulative table, a payload that runs out)
        if (comp_size < 1032 + 4) return RCX_ERROR;
        const u32 declared = le32(comp);
        if (declared > sink_capacity || declared == 0 || declared > RCX_MAX_RANS_STREAM) return RCX_ERROR; // :541, :618
        const u32 rblock = declared < RCX_MIN_BLOCK ? RCX_MIN_BLOCK : declared;
        int rr = stage_stream(c, comp, comp_size, declared);
        if (rr != RCX_OK) return rr;
        c->rans_track = true;
        rr = rcx_decode_blocks_device(c, coder, c->h_in, comp_size, c->h_off, 1, rblock, declared, c->h_out, nullptr);
        c->rans_track = false;
        if (rr != RCX_OK) return rr;
        rr = rcx_ctx_sync_status(c, nullptr, nullptr);
        if (rr == RCX_E_CORRUPT) return RCX_ERROR;
        if (rr != RCX_OK) return rr;
        HIP_TRY(hipMemcpy(dst, c->h_out, declared, hipMemcpyDeviceToHost));
        *dst_size = declared;
        if (request_size) { // what the reference returns: payload bytes consumed (decode) / the symbol count (decode_simd)
            *request_size = declared;
            if (coder == RCX_CODER_RANS) {
                HIP_TRY(hipMemcpy(c->status_host, c->status, 4 * sizeof(u32), hipMemcpyDeviceToHost));
                *request_size = c->status_host[2];
            }
        }
        return RCX_OK;
    }
    if (coder == RCX_CODER_STATIC) {
        // RangeEncoder<T>::decode (cpprcoder.h:460-519): bool.  RCX_OK = true; RCX_ERROR = false, with the
        // symbols written before the failure in dst; a full sink is the caller's to notice (it replays writeByte).
        if (comp_size < 516) return RCX_ERROR;                       // :468-476
        const u32 declared = le32(comp);
        if (declared == 0) return RCX_OK;                            // :481-483
        if (comp_size < 516 + 1 || comp_size - 516 < 5) return RCX_ERROR; // :486-493
        const u64 count = declared < sink_capacity ? declared : sink_capacity;
        if (count > RCX_MAX_STREAM) return RCX_E_ARG;
        if (count == 0) return RCX_OK; // nothing fits: the caller's first writeByte fails
        const u32 block = count < RCX_MIN_BLOCK ? RCX_MIN_BLOCK : (u32)count;
        int r = stage_stream(c, comp, comp_size, count);
        if (r != RCX_OK) return r;
        if (count == declared && count >= RCX_MIN_BLOCK && count <= RCX_MAX_BLOCK && decode_lanes(c, 1) != 1) {
            bool done = false;
            auto quad = [&] {
                hipLaunchKernelGGL(rcx_dec_static_quad_k<RCX_QUAD_DEC_WAVES>, dim3(1), dim3(64 * RCX_QUAD_DEC_WAVES), 0, nullptr, c->h_in, (u64)comp_size,
                                   c->h_off, (u64)1, block, count, c->h_out, c->status, c->redo, 1u);
            };
            if ((r = decode_fast(c, quad, dst, count, dst_size, &done)) != RCX_OK || done) return r;
        }
        hipLaunchKernelGGL(rcx_dec_static_k<true>, dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)comp_size, c->h_off, (u64)1, block, count, c->h_out,
                           c->status, c->status + 2, static_cast<const u32*>(nullptr));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(c->status_host, c->status, 4 * sizeof(u32), hipMemcpyDeviceToHost));
        const u32 short_at = c->status_host[2];
        const u64 produced = short_at < count ? short_at : count;
        if (produced) HIP_TRY(hipMemcpy(dst, c->h_out, produced, hipMemcpyDeviceToHost));
        *dst_size = produced;
        return short_at < count ? RCX_ERROR : RCX_OK;
    }
    if (comp_size < 8) { // cpprcoder.h:878-880
        if (request_size) *request_size = 8;
        return RCX_PENDING;
    }
    const u32 declared = le32(comp);
    const u64 cap16 = sink_capacity;
    const u64 want = declared ? declared : 1; // cpprcoder.h:912: the size test comes after the first writeByte
    const u64 count = want < cap16 ? want : cap16;
    if (count > RCX_MAX_STREAM) return RCX_E_ARG;
    if (count == 0) { // a sink that accepts nothing: the first writeByte fails (cpprcoder.h:909-911)
        if (request_size) *request_size = declared;
        return RCX_PENDING;
    }
    const u32 block = count < RCX_MIN_BLOCK ? RCX_MIN_BLOCK : (u32)count;
    const bool longer = count > RCX_MAX_BLOCK;
    int r = longer ? RCX_OK : ensure_divtab(c, block);
    if (r == RCX_OK) r = stage_stream(c, comp, comp_size, count);
    if (r != RCX_OK) return r;
    if (!longer && count == declared && count >= RCX_MIN_BLOCK && decode_lanes(c, 1) == 4) {
        bool done = false;
        auto quad = [&] {
            hipLaunchKernelGGL(rcx_dec_quad_k<RCX_QUAD_DEC_WAVES>, dim3(1), dim3(64 * RCX_QUAD_DEC_WAVES), 0, nullptr, c->h_in, (u64)comp_size, c->h_off,
                               (u64)1, block, count, c->h_out, c->divq(), c->status, c->redo, 1u);
        };
        if ((r = decode_fast(c, quad, dst, count, dst_size, &done)) != RCX_OK || done) return r;
    }
    if (longer)
        hipLaunchKernelGGL((rcx_dec_adaptive_k<true, true>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)comp_size, c->h_off, (u64)1, block, count, c->h_out,
                           c->divtab(), c->status, c->status + 2, static_cast<const u32*>(nullptr));
    else
        hipLaunchKernelGGL((rcx_dec_adaptive_k<true, false>), dim3(1), dim3(64), 0, nullptr, c->h_in, (u64)comp_size, c->h_off, (u64)1, block, count, c->h_out,
                           c->divtab(), c->status, c->status + 2, static_cast<const u32*>(nullptr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(c->status_host, c->status, 4 * sizeof(u32), hipMemcpyDeviceToHost));
    const u32 short_at = c->status_host[2];
    u64 produced = count;
    int result = RCX_OK;
    if (short_at != 0xFFFFFFFFu && short_at < count) { // input ran dry first (cpprcoder.h:901-903)
        produced = short_at;
        result = RCX_PENDING;
    } else if (want > cap16) { // sink full (cpprcoder.h:909-911)
        result = RCX_PENDING;
    }
    if (result == RCX_PENDING && request_size) *request_size = declared - (u32)produced;
    if (produced) HIP_TRY(hipMemcpy(dst, c->h_out, produced, hipMemcpyDeviceToHost));
    *dst_size = produced;
    return result;
}

int rcx_dstream_create(rcx_ctx* c, rcx_dstream** out)
{
    if (!c || !out) return RCX_E_ARG;
    *out = nullptr;
    HIP_TRY(rcx_enter_device(c->device));
    rcx_dstream* d = new (std::nothrow) rcx_dstream();
    if (!d) return RCX_E_NOMEM;
    d->ctx = c;
    if (d->state.reserve(1) != RCX_OK || d->out.reserve(RCX_DSTREAM_CHUNK) != RCX_OK || d->result.reserve(6) != RCX_OK ||
        d->result_host.reserve(6) != RCX_OK || hipMemset(d->state, 0, sizeof(RcxDState)) != hipSuccess) {
        rcx_dstream_destroy(d);
        return RCX_E_NOMEM;
    }
    *out = d;
    return RCX_OK;
}

void rcx_dstream_destroy(rcx_dstream* d)
{
    if (!d) return;
    if (d->ctx) (void)hipSetDevice(d->ctx->device);
    delete d;
}

int rcx_dstream_decode(rcx_dstream* d, const uint8_t* bytes, uint64_t size, uint8_t* dst, uint64_t dst_cap,
                       uint64_t* produced_now, uint32_t* request_size)
{
    if (!d || !produced_now || (size && !bytes) || (dst_cap && !dst)) return RCX_E_ARG;
    *produced_now = 0;
    if (request_size) *request_size = 0;
    if (d->finished) return RCX_OK;
    HIP_TRY(rcx_enter_device(d->ctx->device));
    if (d->in_bytes == 0 && size < 8) { // cpprcoder.h:877-880: State_Init wants its 8 bytes in one call and keeps nothing
        if (request_size) *request_size = 8;
        return RCX_PENDING;
    }
    if (size) { // append
        if (d->in_bytes + size > d->in.count()) {
            // More room: the new buffer takes only what the decoder has not read yet (it reads all it can, so that is a few
            // bytes unless dst filled up first) -- the stream's past is dropped, and the decoder's memory stays at about twice
            // the largest piece it was ever fed, not the size of the stream.  (A buffer's own growth keeps nothing, and this
            // tail has to survive: a second buffer, the copy, then the two change places.)
            const u64 keep_from = d->consumed > d->in_base ? d->consumed - d->in_base : 0;
            const u64 keep = d->in_bytes - keep_from;
            u64 cap = d->in.count() ? d->in.count() : (1u << 16);
            while (cap < keep + size) cap *= 2;
            DevBuf<u8> bigger;
            if (bigger.reserve(cap) != RCX_OK) return RCX_E_NOMEM;
            if (keep) HIP_TRY(hipMemcpy(bigger, d->in + keep_from, keep, hipMemcpyDeviceToDevice));
            d->in.swap(bigger);
            d->in_base += keep_from;
            d->in_bytes = keep;
        }
        HIP_TRY(hipMemcpy(d->in + d->in_bytes, bytes, size, hipMemcpyHostToDevice));
        d->in_bytes += size;
    }
    u64 made_total = 0;
    for (;;) {
        const u64 room64 = dst_cap - made_total;
        const u32 room = room64 > RCX_DSTREAM_CHUNK ? RCX_DSTREAM_CHUNK : (u32)room64;
        // (the kernel counts from the start of the stream: in[0] is byte in_base of it, and it never looks before what it has read)
        hipLaunchKernelGGL(rcx_dec_resume_k, dim3(1), dim3(64), 0, nullptr, d->state, d->in - d->in_base, d->in_base + d->in_bytes, d->out, room, d->result);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(d->result_host, d->result, 6 * sizeof(u32), hipMemcpyDeviceToHost));
        d->consumed = (u64)d->result_host[4] | ((u64)d->result_host[5] << 32);
        const u32 made = d->result_host[0];
        d->finished = d->result_host[1] != 0;
        d->declared = d->result_host[2];
        d->produced = d->result_host[3];
        if (made) HIP_TRY(hipMemcpy(dst + made_total, d->out, made, hipMemcpyDeviceToHost));
        made_total += made;
        if (d->finished || made < room || made_total == dst_cap) break; // done, input dry, or dst full
    }
    *produced_now = made_total;
    if (d->finished) return RCX_OK;
    if (request_size) *request_size = d->declared - d->produced; // cpprcoder.h:901-903 / :909-911
    return RCX_PENDING;
}

int rcx_estream_create(rcx_ctx* c, uint32_t declared, rcx_estream** out)
{
    if (!c || !out || declared > RCX_MAX_STREAM) return RCX_E_ARG;
    *out = nullptr;
    HIP_TRY(rcx_enter_device(c->device));
    rcx_estream* e = new (std::nothrow) rcx_estream();
    if (!e) return RCX_E_NOMEM;
    e->ctx = c;
    e->declared = declared;
    const u32 block = declared < RCX_MIN_BLOCK ? RCX_MIN_BLOCK : declared;
    e->slot_bytes = declared <= RCX_MAX_BLOCK ? rcx_block_bound(block) : (((u64)declared + declared / 8 + 4096 + 15) & ~(u64)15);
    RcxEState zero;
    memset(&zero, 0, sizeof(zero));
    zero.declared = declared;
    if (e->state.reserve(1) != RCX_OK || e->backup.reserve(1) != RCX_OK || e->slot.reserve(e->slot_bytes + 64) != RCX_OK ||
        e->result.reserve(8) != RCX_OK || e->result_host.reserve(8) != RCX_OK ||
        hipMemcpy(e->state, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) {
        rcx_estream_destroy(e);
        return RCX_E_NOMEM;
    }
    *out = e;
    return RCX_OK;
}

void rcx_estream_destroy(rcx_estream* e)
{
    if (!e) return;
    if (e->ctx) (void)hipSetDevice(e->ctx->device);
    delete e;
}

int rcx_estream_encode(rcx_estream* e, const uint8_t* bytes, uint64_t size, uint8_t* dst, uint64_t dst_cap, uint64_t sink_room,
                       uint64_t* emitted_now, uint32_t* tail_bytes, uint32_t* request_size)
{
    if (!e || !emitted_now || (size && !bytes) || (dst_cap && !dst)) return RCX_E_ARG;
    *emitted_now = 0;
    if (tail_bytes) *tail_bytes = 0;
    if (request_size) *request_size = 0;
    if (e->finished) return RCX_OK;
    if (e->dead) { // the reference's coder is of no use after a full sink either (cpprcoder.h:708-711)
        if (request_size) *request_size = e->declared - e->consumed;
        return RCX_PENDING;
    }
    if (size > (u64)(e->declared - e->consumed)) return RCX_E_ARG; // CPPRCODER_ASSERT, cpprcoder.h:700
    HIP_TRY(rcx_enter_device(e->ctx->device));
    // what this call may change, kept for rcx_estream_rewind: the state, and the stream from the first byte the reference
    // has not written yet (a carry stops there) to a little past what is in memory
    {
        const u64 from = 4 + e->written, upto = 4 + e->pos_hint + 16 < e->slot_bytes ? 4 + e->pos_hint + 16 : e->slot_bytes;
        const u64 span = upto > from ? upto - from : 0;
        const int r = e->tail_backup.reserve_pow2(span, 4096);
        if (r != RCX_OK) return r;
        HIP_TRY(hipMemcpy(e->backup, e->state, sizeof(RcxEState), hipMemcpyDeviceToDevice));
        if (span) HIP_TRY(hipMemcpy(e->tail_backup, e->slot + from, span, hipMemcpyDeviceToDevice));
        e->tail_from = from;
        e->tail_bytes = span;
        e->backup_consumed = e->consumed;
        e->backup_written = e->written;
        e->have_backup = true;
    }
    if (e->in.reserve_pow2(size, 1u << 16) != RCX_OK) return RCX_E_NOMEM;
    if (size) HIP_TRY(hipMemcpy(e->in, bytes, size, hipMemcpyHostToDevice));
    const u32 room = sink_room > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sink_room;
    hipLaunchKernelGGL(rcx_enc_resume_k, dim3(1), dim3(64), 0, nullptr, e->state, e->in, (u32)size, e->slot, (u32)(e->slot_bytes > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : e->slot_bytes), room,
                       e->result);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(e->result_host, e->result, 8 * sizeof(u32), hipMemcpyDeviceToHost));
    const u32 written = e->result_host[0], fail_at = e->result_host[1], finished = e->result_host[2], stream_size = e->result_host[3],
              flush_fails = e->result_host[4], overflow = e->result_host[5];
    if (overflow) return RCX_E_CAPACITY; // (the slot is the bound of a stream of this size: cannot happen)
    u64 now = (u64)written - e->written; // payload bytes the reference passed to writeByte during this call
    int status = RCX_PENDING;
    u32 tail = 0;
    if (fail_at != 0xFFFFFFFFu) { // its sink filled inside symbol fail_at (cpprcoder.h:708-711)
        // it writes byte by byte until writeByte fails, so the sink is exactly full: also the part of the last group (held
        // byte + pending run) that still fitted, which the kernel's count of whole groups does not include
        now = sink_room;
        e->consumed = fail_at;
        e->dead = true;
    } else if (finished) { // cpprcoder.h:744-762: the held byte and the pending run through writeByte, low through write(4)
        const u64 through_write_byte = (u64)stream_size - 8 - e->written;
        if (flush_fails) {
            now = through_write_byte < sink_room ? through_write_byte : sink_room; // finish() gave up; encode() says Success (cpprcoder.h:716)
        } else {
            now = through_write_byte;
            tail = 4;
        }
        e->consumed = e->declared;
        e->finished = true;
        status = RCX_OK;
    } else {
        e->consumed += (u32)size;
    }
    *emitted_now = now + tail;
    if (now + tail > dst_cap) return RCX_E_CAPACITY;
    if (now) HIP_TRY(hipMemcpy(dst, e->slot + 4 + e->written, now, hipMemcpyDeviceToHost));
    if (tail) HIP_TRY(hipMemcpy(dst + now, e->slot + stream_size - 4, 4, hipMemcpyDeviceToHost));
    e->written += now;
    e->pos_hint = e->result_host[6]; // how far the stream reaches in memory: what the next call can change ends a little past it
    if (tail_bytes) *tail_bytes = tail;
    if (status == RCX_PENDING && request_size) *request_size = e->declared - e->consumed;
    return status;
}

// Back to before the last rcx_estream_encode call.  For a sink that only tells by failing how much room it has: encode with
// no limit, hand the bytes on, and if the sink fails after k of them rewind and encode the same piece with sink_room = k to
// learn which symbol the reference was coding then.
int rcx_estream_rewind(rcx_estream* e)
{
    if (!e || !e->have_backup) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(e->ctx->device));
    HIP_TRY(hipMemcpy(e->state, e->backup, sizeof(RcxEState), hipMemcpyDeviceToDevice));
    if (e->tail_bytes) HIP_TRY(hipMemcpy(e->slot + e->tail_from, e->tail_backup, e->tail_bytes, hipMemcpyDeviceToDevice));
    e->consumed = e->backup_consumed;
    e->written = e->backup_written;
    e->dead = false;
    e->finished = false;
    e->have_backup = false;
    return RCX_OK;
}

} // extern "C"
