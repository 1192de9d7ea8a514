// rcx_bwt_api.hpp -- the block sort's calls of include/rcx.h (blksort.h): whole 32 KiB blocks are transformed, what is
// left over is copied (blksort.h:440-462).  The kernels are rcx_bwt.hpp and rcx_bwt_tie.hpp.
#pragma once
#include "rcx_host.hpp"

namespace
{
int bwt_host(rcx_ctx* c, bool forward, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size)
{
    if (!c || !dst_size || (n && (!src || !dst))) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    const u64 out = forward ? rcx_bwt_encode_bound(n) : rcx_bwt_decoded_size(n);
    *dst_size = out;
    if (out > dst_cap) return RCX_E_CAPACITY;
    if (n == 0) return RCX_OK;
    int r = reserve_staging(c, n, out, 0);
    if (r != RCX_OK) return r;
    // Chunks of 1024 whole blocks (32 MiB); what is left over after the last whole block travels with the last chunk.
    // These kernels take blocks off a counter with one workgroup per CU, so a chunk's kernels take the chunk's share of
    // the time and follow each other on ONE stream (they also share the context's list of periodic blocks).
    const u64 unit_in = forward ? RCX_BWT_BLOCK : RCX_BWT_ENCODED, unit_out = forward ? RCX_BWT_ENCODED : RCX_BWT_BLOCK;
    const u64 blocks = n / unit_in, cb = 1024;
    const u64 chunks = (blocks + cb - 1) / cb;
    if (c->pipe) c->pipe->bwt_ties_valid = false;
    if (chunks < 2 || getenv("RCX_HOST_SERIAL")) {
        HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
        r = forward ? rcx_bwt_encode_device(c, c->h_in, n, c->h_out, out, nullptr) : rcx_bwt_decode_device(c, c->h_in, n, c->h_out, out, nullptr);
        if (r != RCX_OK) return r;
        r = rcx_ctx_sync_status(c, nullptr, nullptr);
        if (r != RCX_OK) return r;
        HIP_TRY(hipMemcpy(dst, c->h_out, out, hipMemcpyDeviceToHost));
        return RCX_OK;
    }
    HostPipe* p = nullptr;
    if ((r = host_pipe_get(c, &p)) != RCX_OK) return r;
    if ((r = host_pipe_words(p, chunks + 1)) != RCX_OK) return r;
    if ((r = rcx_bwt_reserve(c, forward ? n : 0)) != RCX_OK) return r;
    auto in_bytes = [&](u64 k) { return k + 1 < chunks ? cb * unit_in : n - k * cb * unit_in; };
    auto out_bytes = [&](u64 k) { return k + 1 < chunks ? cb * unit_out : out - k * cb * unit_out; };
    HostJob job;
    job.chunks = chunks;
    job.work_streams = 1;
    job.in = [&](u64 k) -> HostSpan { return HostSpan{src + k * cb * unit_in, c->h_in + k * cb * unit_in, in_bytes(k)}; };
    job.launch = [&](u64 k, hipStream_t s) -> int {
        const u8* from = c->h_in + k * cb * unit_in;
        u8* to = c->h_out + k * cb * unit_out;
        const int e = forward ? rcx_bwt_encode_device(c, from, in_bytes(k), to, out_bytes(k), s) : rcx_bwt_decode_device(c, from, in_bytes(k), to, out_bytes(k), s);
        if (e != RCX_OK || !forward) return e;
        // how many of the chunk's blocks were periodic (rcx_bwt_last_ties adds the chunks up)
        p->words[k] = 0;
        return hipMemcpyAsync(p->words + k, c->ties, sizeof(u32), hipMemcpyDeviceToHost, s) == hipSuccess ? RCX_OK : RCX_E_HIP;
    };
    job.out = [&](u64 k, HostSpan* span) -> int {
        *span = HostSpan{c->h_out + k * cb * unit_out, dst + k * cb * unit_out, out_bytes(k)};
        return RCX_OK;
    };
    job.caller_in = src;
    job.caller_out = dst;
    r = host_run(c, p, job);
    const int latched = rcx_ctx_sync_status(c, nullptr, nullptr);
    if (r != RCX_OK) return r;
    if (latched != RCX_OK) return latched;
    if (forward) {
        p->bwt_ties = 0;
        for (u64 k = 0; k < chunks; ++k) p->bwt_ties += p->words[k];
        p->bwt_ties_valid = true;
    }
    return RCX_OK;
}
} // namespace

extern "C" {

uint64_t rcx_bwt_encode_bound(uint64_t n)
{
    const u64 blocks = n / RCX_BWT_BLOCK;
    return blocks * RCX_BWT_ENCODED + (n - blocks * RCX_BWT_BLOCK);
}

uint64_t rcx_bwt_decode_bound(uint64_t n)
{
    const u64 blocks = n / RCX_BWT_BLOCK;
    return blocks * RCX_BWT_BLOCK + (n - blocks * RCX_BWT_BLOCK);
}

uint64_t rcx_bwt_decoded_size(uint64_t n)
{
    const u64 blocks = n / RCX_BWT_ENCODED;
    return blocks * RCX_BWT_BLOCK + (n - blocks * RCX_BWT_ENCODED);
}

int rcx_bwt_reserve(rcx_ctx* c, uint64_t n)
{
    if (!c) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (c->bwt_atomic < 0) { // the context's first block-sort call
        if (allow_lds(c, &rcx_bwt_fwd_k<false>, RCX_BWT_FWD_LDS) != RCX_OK || allow_lds(c, &rcx_bwt_fwd_k<true>, RCX_BWT_FWD_LDS) != RCX_OK ||
            allow_lds(c, &rcx_bwt_inv_k<false>, RCX_BWT_INV_LDS) != RCX_OK || allow_lds(c, &rcx_bwt_inv_k<true>, RCX_BWT_INV_LDS) != RCX_OK ||
            allow_lds(c, &rcx_bwt_tie_k, RCX_BWT_TIE_LDS) != RCX_OK)
            return RCX_E_HIP;
        // The counting passes rank the keys of a batch with ballots (documented behaviour only).  RCX_BWT_MATCH=atomic asks
        // for one ds_add_rtn_u32 per key instead (5-25 % faster), which is only a stable rank if the LDS serves the lanes
        // of one instruction in ascending lane order -- the ISA manual does not say so, so it is opt-in, and even then only
        // taken if a short check on this device (rcx_bwt_lds_order_k, once per device and process) finds it to hold.
        const char* want = getenv("RCX_BWT_MATCH");
        int atomic = 0;
        if (want && !strcmp(want, "atomic")) {
            // (one answer per device and process: 0.3 ms the first time; a benign race if two threads ask at once)
            static int known[64]; // 0 = not asked, 1 = lane order holds, 2 = it does not
            int& answer = known[c->device & 63];
            if (answer == 0) {
                u32 bad = 1;
                const int rr = c->ties.reserve(8);
                if (rr != RCX_OK) return rr;
                HIP_TRY(hipMemset(c->ties, 0, sizeof(u32)));
                hipLaunchKernelGGL(rcx_bwt_lds_order_k, dim3(4), dim3(1024), 0, nullptr, 512u, c->ties);
                HIP_TRY(hipMemcpy(&bad, c->ties, sizeof(u32), hipMemcpyDeviceToHost));
                answer = bad == 0 ? 1 : 2;
            }
            atomic = answer == 1;
        }
        c->bwt_atomic = atomic;
    }
    return c->ties.reserve(RCX_BWT_TIES_HEAD + 2 * (n / RCX_BWT_BLOCK) + 2);
}

int rcx_bwt_encode_device(rcx_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t dst_cap, void* stream)
{
    if (!c || (n && (!d_src || !d_dst))) return RCX_E_ARG;
    if (dst_cap < rcx_bwt_encode_bound(n)) return RCX_E_CAPACITY;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int r = rcx_bwt_reserve(c, n);
    if (r != RCX_OK) return r;
    const u64 blocks = n / RCX_BWT_BLOCK;
    const u8* src = static_cast<const u8*>(d_src);
    u8* dst = static_cast<u8*>(d_dst);
    if (blocks >> 32) return RCX_E_ARG; // (the block counters are 32 bits: 128 TiB)
    if (c->pipe) c->pipe->bwt_ties_valid = false;
    HIP_TRY(hipMemsetAsync(c->ties, 0, 2 * sizeof(u32), s)); // the tie count and the forward kernel's block counter
    if (blocks) {
        Timed t(c, s, RCX_T_BWT_FORWARD);
        const u32 grid = (u32)(blocks < (u64)c->cus ? blocks : (u64)c->cus); // one workgroup per CU, blocks off a counter
        if (c->bwt_atomic == 1) hipLaunchKernelGGL(rcx_bwt_fwd_k<true>, dim3(grid), dim3(RCX_BWT_THREADS), RCX_BWT_FWD_LDS, s, src, blocks, dst, c->ties, c->status);
        else hipLaunchKernelGGL(rcx_bwt_fwd_k<false>, dim3(grid), dim3(RCX_BWT_THREADS), RCX_BWT_FWD_LDS, s, src, blocks, dst, c->ties, c->status);
        // periodic blocks (rotations that tie) get the row index the reference's sort would leave; usually none
        const u64 most = 2ull * (u64)c->cus;
        hipLaunchKernelGGL(rcx_bwt_tie_k, dim3((u32)(blocks < most ? blocks : most)), dim3(64), RCX_BWT_TIE_LDS, s, src, dst,
                           static_cast<const u32*>(c->ties), c->status);
    }
    const u64 rest = n - blocks * RCX_BWT_BLOCK;
    if (rest) HIP_TRY(hipMemcpyAsync(dst + blocks * RCX_BWT_ENCODED, src + blocks * RCX_BWT_BLOCK, rest, hipMemcpyDeviceToDevice, s));
    return LAUNCHED();
}

int rcx_bwt_decode_device(rcx_ctx* c, const void* d_src, uint64_t n, void* d_dst, uint64_t dst_cap, void* stream)
{
    if (!c || (n && (!d_src || !d_dst))) return RCX_E_ARG;
    if (dst_cap < rcx_bwt_decoded_size(n)) return RCX_E_CAPACITY;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int r = rcx_bwt_reserve(c, 0);
    if (r != RCX_OK) return r;
    const u64 blocks = n / RCX_BWT_ENCODED;
    if (blocks >> 32) return RCX_E_ARG;
    HIP_TRY(hipMemsetAsync(c->ties + 2, 0, sizeof(u32), s)); // the inverse kernel's block counter
    const u8* src = static_cast<const u8*>(d_src);
    u8* dst = static_cast<u8*>(d_dst);
    if (blocks) {
        Timed t(c, s, RCX_T_BWT_INVERSE);
        const u32 grid = (u32)(blocks < (u64)c->cus ? blocks : (u64)c->cus);
        if (c->bwt_atomic == 1) hipLaunchKernelGGL(rcx_bwt_inv_k<true>, dim3(grid), dim3(RCX_BWT_THREADS), RCX_BWT_INV_LDS, s, src, blocks, dst, c->ties + 2, c->status);
        else hipLaunchKernelGGL(rcx_bwt_inv_k<false>, dim3(grid), dim3(RCX_BWT_THREADS), RCX_BWT_INV_LDS, s, src, blocks, dst, c->ties + 2, c->status);
    }
    const u64 rest = n - blocks * RCX_BWT_ENCODED;
    if (rest) HIP_TRY(hipMemcpyAsync(dst + blocks * RCX_BWT_BLOCK, src + blocks * RCX_BWT_ENCODED, rest, hipMemcpyDeviceToDevice, s));
    return LAUNCHED();
}

int rcx_bwt_encode(rcx_ctx* c, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size)
{
    return bwt_host(c, true, src, n, dst, dst_cap, dst_size);
}

int rcx_bwt_decode(rcx_ctx* c, const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size)
{
    return bwt_host(c, false, src, n, dst, dst_cap, dst_size);
}

int rcx_bwt_last_ties(rcx_ctx* c, uint64_t* count)
{
    if (!c || !count) return RCX_E_ARG;
    *count = 0;
    if (!c->ties) return RCX_OK;
    if (c->pipe && c->pipe->bwt_ties_valid) { // the last forward call was a host-buffer call made in chunks
        *count = c->pipe->bwt_ties;
        return RCX_OK;
    }
    HIP_TRY(rcx_enter_device(c->device));
    HIP_TRY(hipDeviceSynchronize());
    u32 v = 0;
    HIP_TRY(hipMemcpy(&v, c->ties, sizeof(u32), hipMemcpyDeviceToHost));
    *count = v;
    return RCX_OK;
}

} // extern "C"
