// rcx_api.hip -- the C ABI of include/rcx.h on top of the gfx950 kernels: the context's calls and the many-block calls
// here, the rest by concern in the headers below (one translation unit).
//
// Host-side restatement of the reference's driver code path: where
// test/main.cpp:321-344 constructs a MemoryStream and a coder per buffer and
// calls initialize/encode/decode, a caller here makes one rcx_ctx per GPU and
// calls rcx_encode_blocks_device / rcx_decode_blocks_device per buffer.
#include "rcx_ctx.hpp"      // the context, its scratch, what every launch site uses
#include "rcx_launch.hpp"   // which kernels code a set of blocks, in which shape
#include "rcx_host.hpp"     // the host-buffer calls' pipeline
#include "rcx_items.hpp"    // the item calls
#include "rcx_streams.hpp"  // single streams, whole and resumable
#include "rcx_bwt_api.hpp"  // the block sort
#include "rcx_crc_api.hpp"  // CRC-32 per block or item
#include "rcx_stats_api.hpp" // byte counts and order-0 cost per block or item (include/rcx_stats.h)
#include "rcx_stored_api.hpp" // stored blocks: mix behind the block encode call, decode of any picks (include/rcx_stored.h)
#include "rcx_stored_items_api.hpp" // stored items: the mix behind the item encode call (include/rcx_stored_items.h)
#include "rcx_typed_api.hpp" // the byte-plane filter and the delta predictor in front of it (include/rcx_planes.h, rcx_predict.h)
#include "rcx_typed_items_api.hpp" // the same per item: a width and a predictor of its own for every buffer (include/rcx_typed_items.h)
#include "rcx_base_api.hpp" // residuals against a base buffer in front of the plane filter (include/rcx_base.h)
#include "rcx_base_items_api.hpp" // the same per item: an op and a base span of its own for every buffer (include/rcx_base_items.h)
#include "rcx_typed_stats_api.hpp" // the cost of every candidate predictor and op of every item, in one pass (include/rcx_typed_stats.h)
#include "rcx_picks_api.hpp" // item decode planned on the device: every table in HBM, capturable (include/rcx_picks.h)
#include "rcx_typed_picks_api.hpp" // the typed join per item planned on the device, capturable (include/rcx_typed_picks.h)
#include "rcx_base_picks_api.hpp" // the base join per item planned on the device, capturable (include/rcx_base_picks.h)
#include "rcx_encode_picks_api.hpp" // item encode planned on the device: every table in HBM, capturable (include/rcx_encode_picks.h)
#include "rcx_typed_split_picks_api.hpp" // the typed split per item planned on the device, capturable (include/rcx_typed_split_picks.h)

extern "C" {

int rcx_version(void) { return RCX_VERSION; }

const char* rcx_status_string(int status)
{
    switch (status) {
    case RCX_OK: return "success";
    case RCX_PENDING: return "pending";
    case RCX_ERROR: return "error";
    case RCX_E_ARG: return "bad argument";
    case RCX_E_CAPACITY: return "destination too small";
    case RCX_E_CORRUPT: return "corrupt or truncated block stream";
    case RCX_E_HIP: return "HIP runtime error";
    case RCX_E_NOMEM: return "out of memory";
    case RCX_E_COMM: return "RCCL error";
    default: return "unknown status";
    }
}

uint64_t rcx_block_count(uint64_t n, uint32_t block) { return block ? (n + block - 1) / block : 0; }

// Worst case of one adaptive block: n + (255/2)*log2(n)/8 (estimator regret) + the truncation loss of
// t = range/total, which is < log2(1 + 1/t) bits per symbol: < n/64 bytes while total <= 2^20 (t >= 16), and up to
// one bit per symbol as the total approaches 2^24 (t >= 1); plus the 9 framing bytes.
// The static coder needs 521 + n + slack.  Rounded to 16 so slots keep 16-byte alignment.
uint64_t rcx_block_bound(uint32_t block)
{
    uint64_t b = (uint64_t)block + block / 32 + 2048;
    if (block > (1u << 20)) b += block / 8;
    return (b + 15) & ~(uint64_t)15;
}

uint64_t rcx_encode_bound(uint64_t n, uint32_t block) { return rcx_block_count(n, block) * rcx_block_bound(block) + 16; }

uint64_t rcx_block_bound_for(int coder, uint32_t block)
{
    if (!is_rans(coder)) return rcx_block_bound(block);
    return (2 * (uint64_t)block + 1032 + 64 + 15) & ~(uint64_t)15; // cppans.h:492-495 + 64, see rcx.h
}

uint64_t rcx_encode_bound_for(int coder, uint64_t n, uint32_t block) { return rcx_block_count(n, block) * rcx_block_bound_for(coder, block) + 16; }

int rcx_ctx_create(int device, rcx_ctx** out)
{
    if (!out) return RCX_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return RCX_E_HIP; // no CPU fallback: fail loudly
    if (device < 0 || device >= count) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(device));
    rcx_ctx* c = new (std::nothrow) rcx_ctx();
    if (!c) return RCX_E_NOMEM;
    c->device = device;
#if defined(RCX_WITH_VARIANTS) // (the diagnostic build with csrc/variants/: the superseded kernels can be chosen too)
    const bool variants = true;
#else
    const bool variants = false;
#endif
    if (const char* v = getenv("RCX_LANES_PER_BLOCK")) c->lanes_per_block = (atoi(v) == 1 || atoi(v) == 4 || (variants && atoi(v) == 8)) ? atoi(v) : 0;
    if (const char* v = getenv("RCX_WIDE_WG")) c->wide_wg = atoi(v) ? 1 : 0;
    if (const char* v = getenv("RCX_ENC_VARIANT")) c->enc_variant = (atoi(v) == 0 || atoi(v) == 3 || (variants && (atoi(v) == 1 || atoi(v) == 2))) ? atoi(v) : 3;
    if (const char* v = getenv("RCX_ENC_LANES")) c->enc_lanes = atoi(v) >= 1 && atoi(v) <= 64 ? atoi(v) : 0;
    if (const char* v = getenv("RCX_DEC_QUADS")) { const int q = atoi(v); c->dec_quads = (q == 1 || q == 2 || q == 4 || q == 8 || q == 16) ? q : 0; }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = cus;
    }
    if (c->status.reserve(4) != RCX_OK || c->status_host.reserve(4) != RCX_OK) {
        rcx_ctx_destroy(c);
        return RCX_E_NOMEM;
    }
    const u32 init[2] = {0u, 0xFFFFFFFFu};
    if (hipMemcpy(c->status, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
        rcx_ctx_destroy(c);
        return RCX_E_HIP;
    }
    *out = c;
    return RCX_OK;
}

void rcx_ctx_destroy(rcx_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& p : c->pending) c->pool.push_back(p);
    for (auto& p : c->pool) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    host_pipe_destroy(c->pipe);
    delete c; // (and with it every buffer it owns)
}

int rcx_ctx_reserve(rcx_ctx* c, uint64_t n, uint32_t block)
{
    if (!c || !block_ok(block)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return reserve(c, n, block);
}

int rcx_ctx_reserve_for(rcx_ctx* c, int coder, uint64_t n, uint32_t block)
{
    if (!c || !block_ok(block) || !coder_ok(coder)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    return reserve(c, n, block, coder);
}

int rcx_ctx_sync_status(rcx_ctx* c, void* stream, uint64_t* first_bad_block)
{
    if (!c) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    HIP_TRY(hipMemcpyAsync(c->status_host, c->status, 2 * sizeof(u32), hipMemcpyDeviceToHost, s));
    const u32 init[2] = {0u, 0xFFFFFFFFu};
    HIP_TRY(hipStreamSynchronize(s));
    const u32 flags = c->status_host[0], bad = c->status_host[1];
    if (flags) {
        HIP_TRY(hipMemcpyAsync(c->status, init, sizeof(init), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (first_bad_block) *first_bad_block = bad;
    if (flags & RCX_ST_CORRUPT) return RCX_E_CORRUPT;
    if (flags & RCX_ST_CAPACITY) return RCX_E_CAPACITY;
    return RCX_OK;
}

int rcx_encode_blocks_device(rcx_ctx* c, int coder, const void* d_src, uint64_t n, uint32_t block,
                             void* d_dst, uint64_t dst_cap, uint64_t* d_offsets, void* stream)
{
    if (!c || !block_ok(block) || !d_offsets || (n && (!d_src || !d_dst))) return RCX_E_ARG;
    if (!coder_ok(coder)) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    const u64 nblocks = rcx_block_count(n, block);
    if (nblocks == 0) return hipMemsetAsync(d_offsets, 0, sizeof(u64), s) == hipSuccess ? RCX_OK : RCX_E_HIP;
    if (nblocks > 0x7FFFFFFFull) return RCX_E_ARG; // grid.x limit with 8 blocks per workgroup to spare
    int r = reserve(c, n, block, coder);
    if (r != RCX_OK) return r;
    return encode_range(c, coder, d_src, n, block, d_dst, dst_cap, d_offsets, s, ScratchRange{});
}

int rcx_decode_blocks_device(rcx_ctx* c, int coder, const void* d_comp, uint64_t comp_size,
                             const uint64_t* d_offsets, uint64_t nblocks, uint32_t block,
                             uint64_t n, void* d_dst, void* stream)
{
    if (!c || !block_ok(block) || (nblocks && (!d_comp || !d_offsets || !d_dst))) return RCX_E_ARG;
    if (!coder_ok(coder)) return RCX_E_ARG;
    if (nblocks != rcx_block_count(n, block)) return RCX_E_ARG;
    if (nblocks == 0) return RCX_OK;
    if (nblocks > 0x7FFFFFFFull) return RCX_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(rcx_enter_device(c->device));
    if (!is_rans(coder)) {
        int r = ensure_divtab(c, block);
        if (r != RCX_OK) return r;
        if ((r = ensure_redo(c, nblocks)) != RCX_OK) return r; // no-op after rcx_ctx_reserve
    }
    return decode_range(c, coder, d_comp, comp_size, d_offsets, nblocks, block, n, d_dst, s, ScratchRange{});
}

int rcx_encode_blocks(rcx_ctx* c, int coder, const uint8_t* src, uint64_t n, uint32_t block,
                      uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* offsets)
{
    if (!c || !block_ok(block) || !dst_size || (n && (!src || !dst))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    if (!coder_ok(coder)) return RCX_E_ARG;
    const u64 nblocks = rcx_block_count(n, block);
    if (nblocks > 0x7FFFFFFFull) return RCX_E_ARG;
    const u64 bound = rcx_encode_bound_for(coder, n, block);
    const u64 cb = host_chunk_blocks(block, false, nblocks);
    const u64 chunks = (nblocks + cb - 1) / cb;
    int r = reserve_staging(c, n, bound, nblocks + chunks + 1);
    if (r != RCX_OK) return r;
    if (chunks < 2 || getenv("RCX_HOST_SERIAL")) { // one chunk: nothing to overlap
        if (n) HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
        r = rcx_encode_blocks_device(c, coder, c->h_in, n, block, c->h_out, bound, c->h_off, nullptr);
        if (r != RCX_OK) return r;
        r = rcx_ctx_sync_status(c, nullptr, nullptr);
        if (r != RCX_OK) return r;
        u64 total = 0;
        HIP_TRY(hipMemcpy(&total, c->h_off + nblocks, sizeof(u64), hipMemcpyDeviceToHost));
        *dst_size = total;
        if (offsets) HIP_TRY(hipMemcpy(offsets, c->h_off, (nblocks + 1) * sizeof(u64), hipMemcpyDeviceToHost));
        if (total > dst_cap) return RCX_E_CAPACITY;
        if (total) HIP_TRY(hipMemcpy(dst, c->h_out, total, hipMemcpyDeviceToHost));
        return RCX_OK;
    }
    // Chunks of `cb` blocks.  Chunk k is encoded into its own part of the device buffer (at its first block's slot
    // offset) with its own table, which comes back with it; where it goes in `dst` is known once the chunks before it
    // are: the drainers add the sizes up as the chunks finish.
    HostPipe* p = nullptr;
    if ((r = host_pipe_get(c, &p)) != RCX_OK) return r;
    if ((r = host_pipe_words(p, nblocks + chunks + 1)) != RCX_OK) return r;
    if ((r = reserve(c, n, block, coder)) != RCX_OK) return r;
    const u64 slot = rcx_block_bound_for(coder, block);
    u64 running = 0;
    bool fits = true;
    HostJob job;
    job.chunks = chunks;
    job.in = [&](u64 k) -> HostSpan {
        const u64 at = k * cb * block;
        return HostSpan{src + at, c->h_in + at, (n - at < cb * block) ? n - at : cb * block};
    };
    job.launch = [&](u64 k, hipStream_t s) -> int {
        const u64 b0 = k * cb, nb = (nblocks - b0 < cb) ? nblocks - b0 : cb;
        const u64 at = b0 * block, len = (n - at < cb * block) ? n - at : cb * block;
        const int e = encode_range(c, coder, c->h_in + at, len, block, c->h_out + b0 * slot, nb * slot, c->h_off + b0 + k, s, ScratchRange{b0, true});
        if (e != RCX_OK) return e;
        return hipMemcpyAsync(p->words + b0 + k, c->h_off + b0 + k, (nb + 1) * sizeof(u64), hipMemcpyDeviceToHost, s) == hipSuccess ? RCX_OK : RCX_E_HIP;
    };
    job.out = [&](u64 k, HostSpan* span) -> int {
        const u64 b0 = k * cb, nb = (nblocks - b0 < cb) ? nblocks - b0 : cb;
        const u64* rel = p->words + b0 + k;
        if (offsets)
            for (u64 i = 0; i < nb; ++i) offsets[b0 + i] = running + rel[i];
        const u64 bytes = rel[nb];
        if (bytes > nb * slot || running + bytes > dst_cap) fits = false; // (a slot overflow is latched on the device as well)
        *span = fits ? HostSpan{c->h_out + b0 * slot, dst + running, bytes} : HostSpan{};
        running += bytes;
        return RCX_OK;
    };
    job.work_streams = 2; // (measured: a third encode chunk in flight gains nothing and delays the copies back)
    job.caller_in = src;
    job.caller_out = dst;
    r = host_run(c, p, job);
    const int latched = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (getenv("RCX_DEBUG") && (r != RCX_OK || latched != RCX_OK)) fprintf(stderr, "rcx: host encode: pipeline %d, latched status %d\n", r, latched);
    if (r != RCX_OK) return r;
    if (latched != RCX_OK) return latched;
    *dst_size = running;
    if (offsets) offsets[nblocks] = running;
    return fits ? RCX_OK : RCX_E_CAPACITY;
}

int rcx_decode_blocks(rcx_ctx* c, int coder, const uint8_t* comp, uint64_t comp_size,
                      const uint64_t* offsets, uint64_t nblocks, uint32_t block,
                      uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size)
{
    if (!c || !block_ok(block) || !dst_size || (nblocks && (!comp || !offsets || !dst))) return RCX_E_ARG;
    if (!coder_ok(coder) || nblocks > 0x7FFFFFFFull) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    *dst_size = 0;
    if (nblocks == 0) return RCX_OK;
    if (offsets[nblocks] > comp_size || offsets[nblocks] < offsets[nblocks - 1] || offsets[nblocks] - offsets[nblocks - 1] < 4)
        return RCX_E_CORRUPT;
    // the last block's declared size fixes n (every earlier block is full)
    const uint8_t* lastp = comp + offsets[nblocks - 1];
    const u64 last_len = le32(lastp);
    if (last_len == 0 || last_len > block) return RCX_E_CORRUPT;
    const u64 n = (nblocks - 1) * (u64)block + last_len;
    if (n > dst_cap) return RCX_E_CAPACITY;
    int r = reserve_staging(c, comp_size, n, nblocks + 1);
    if (r != RCX_OK) return r;
    const u64 cb = host_chunk_blocks(block, true, nblocks);
    const u64 chunks = (nblocks + cb - 1) / cb;
    if (chunks < 2 || getenv("RCX_HOST_SERIAL")) {
        HIP_TRY(hipMemcpy(c->h_in, comp, comp_size, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->h_off, offsets, (nblocks + 1) * sizeof(u64), hipMemcpyHostToDevice));
        r = rcx_decode_blocks_device(c, coder, c->h_in, comp_size, c->h_off, nblocks, block, n, c->h_out, nullptr);
        if (r != RCX_OK) return r;
        r = rcx_ctx_sync_status(c, nullptr, nullptr);
        if (r != RCX_OK) return r;
        HIP_TRY(hipMemcpy(dst, c->h_out, n, hipMemcpyDeviceToHost));
        *dst_size = n;
        return RCX_OK;
    }
    // Chunks of `cb` blocks: a chunk's streams are one stretch of `comp` (the table says which), and they keep their
    // place in the device copy, so the table goes over once and as it is.
    for (u64 b = 0; b < nblocks; ++b)
        if (offsets[b] > offsets[b + 1]) return RCX_E_CORRUPT; // (the host has the table: a chunk is offsets[b0] .. offsets[b1] of `comp`)
    HostPipe* p = nullptr;
    if ((r = host_pipe_get(c, &p)) != RCX_OK) return r;
    if (!is_rans(coder)) {
        if ((r = ensure_divtab(c, block)) != RCX_OK) return r;
        if ((r = ensure_redo(c, nblocks)) != RCX_OK) return r;
    }
    HIP_TRY(hipMemcpy(c->h_off, offsets, (nblocks + 1) * sizeof(u64), hipMemcpyHostToDevice));
    HostJob job;
    job.chunks = chunks;
    job.in = [&](u64 k) -> HostSpan {
        const u64 b0 = k * cb, b1 = (b0 + cb < nblocks) ? b0 + cb : nblocks;
        return HostSpan{comp + offsets[b0], c->h_in + offsets[b0], offsets[b1] - offsets[b0]};
    };
    job.launch = [&](u64 k, hipStream_t s) -> int {
        const u64 b0 = k * cb, nb = (nblocks - b0 < cb) ? nblocks - b0 : cb;
        const u64 at = b0 * block, len = (n - at < cb * block) ? n - at : cb * block;
        return decode_range(c, coder, c->h_in, comp_size, c->h_off + b0, nb, block, len, c->h_out + at, s, ScratchRange{b0, true});
    };
    job.out = [&](u64 k, HostSpan* span) -> int {
        const u64 at = k * cb * block;
        *span = HostSpan{c->h_out + at, dst + at, (n - at < cb * block) ? n - at : cb * block};
        return RCX_OK;
    };
    job.decode = true;
    job.caller_in = comp;
    job.caller_out = dst;
    r = host_run(c, p, job);
    const int latched = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (r != RCX_OK) return r;
    if (latched != RCX_OK) return latched;
    *dst_size = n;
    return RCX_OK;
}

#if defined(RCX_STAMP_DEC)
int rcx_debug_dec_stamps(unsigned long long* out8)
{
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(rcx_dec_stamp_out), 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#if defined(RCX_BWT_STAMP)
int rcx_debug_bwt_stamps(unsigned long long* out16, int reset)
{
    static const unsigned long long zero[16] = {};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(rcx_bwt_stamp_out), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(rcx_bwt_stamp_out), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif
#if defined(RCX_STAMP)
int rcx_debug_stamps(unsigned long long* out16)
{
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(rcx_stamp_out), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

int rcx_ctx_last_redo(rcx_ctx* c, uint64_t nblocks, uint64_t* count)
{
    if (!c || !count) return RCX_E_ARG;
    *count = 0;
    if (nblocks == 0 || !c->redo) return RCX_OK;
    if (nblocks > c->redo.count()) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<u32> host(nblocks);
    HIP_TRY(hipMemcpy(host.data(), c->redo, nblocks * sizeof(u32), hipMemcpyDeviceToHost));
    for (u64 i = 0; i < nblocks; ++i) *count += host[i] != 0;
    return RCX_OK;
}

int rcx_ctx_set_timing(rcx_ctx* c, int enabled)
{
    if (!c) return RCX_E_ARG;
    c->timing = enabled != 0;
    return RCX_OK;
}

int rcx_ctx_get_timing(rcx_ctx* c, double* ms, uint64_t* launches, int reset)
{
    if (!c) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    for (auto& p : c->pending) {
        float t = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
            c->ms[p.what] += t;
            c->launches[p.what] += 1;
        }
        c->pool.push_back(p);
    }
    c->pending.clear();
    for (int i = 0; i < RCX_T_COUNT; ++i) {
        if (ms) ms[i] = c->ms[i];
        if (launches) launches[i] = c->launches[i];
        if (reset) {
            c->ms[i] = 0;
            c->launches[i] = 0;
        }
    }
    return RCX_OK;
}

} // extern "C"
