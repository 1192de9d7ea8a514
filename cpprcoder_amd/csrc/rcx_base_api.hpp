// rcx_base_api.hpp -- the calls of include/rcx_base.h, residuals against a base buffer in front of the coders: one launch per
// call, of rcx_base_k (rcx_base.hpp).
//
// Nothing of the context is used but its device and compute-unit count: no scratch, no table, no latch, nothing to
// reserve, so the device calls can be captured.  The host-buffer calls go through the staging buffers of the other
// host-buffer calls; the input buffer holds the source and, from the next 16-byte border on, the base.
#pragma once

#include "../../include/rcx_base.h"
#include "rcx_base.hpp"
#include "rcx_ctx.hpp"

namespace
{

typedef void (*BaseKernel)(const u8*, const u8*, u8*, u64, u32, u64);

// The grid of rcx_base_k: a fixed one, four workgroups (16 waves) to a compute unit, that loops; fewer where there is
// less to do, and never none (the bytes behind the last whole unit need a workgroup).
dim3 base_grid(const rcx_ctx* c, u64 n, u32 width, u32 block, u64 nfull)
{
    const u64 per = (u64)RCX_BASE_ROWS(width) * RCX_BASE_THREADS;
    u64 units = n >> 4, bytewise = 15; // width 1: one run of units, at most 15 bytes behind it
    if (width > 1) {
        const u64 rest_last = n - nfull * width * block;
        units = nfull * (block >> 4) + (rest_last / width >> 4);
        bytewise = nfull * ((block & 15u) * width) + 17ull * width; // (at most: the last superblock's is below 17 * width)
    }
    u64 want = (units + per - 1) / per;
    if (want < (bytewise + RCX_BASE_THREADS - 1) / RCX_BASE_THREADS) want = (bytewise + RCX_BASE_THREADS - 1) / RCX_BASE_THREADS;
    const u64 most = 4ull * (u64)c->cus;
    return dim3((u32)(want < most ? want : most));
}

template <bool JOIN>
int base_launch(rcx_ctx* c, const u8* src, const u8* ref, u64 n, u32 width, u32 block, u32 op, u8* dst, hipStream_t s)
{
    static constexpr BaseKernel table[4][3] = {
        {rcx_base_k<1, JOIN, 0>, rcx_base_k<1, JOIN, 1>, rcx_base_k<1, JOIN, 2>},
        {rcx_base_k<2, JOIN, 0>, rcx_base_k<2, JOIN, 1>, rcx_base_k<2, JOIN, 2>},
        {rcx_base_k<4, JOIN, 0>, rcx_base_k<4, JOIN, 1>, rcx_base_k<4, JOIN, 2>},
        {rcx_base_k<8, JOIN, 0>, rcx_base_k<8, JOIN, 1>, rcx_base_k<8, JOIN, 2>},
    };
    const BaseKernel kernel = table[width == 1 ? 0 : width == 2 ? 1 : width == 4 ? 2 : 3][op];
    const u64 nfull = n / ((u64)width * block);
    hipLaunchKernelGGL(kernel, base_grid(c, n, width, block, nfull), dim3(RCX_BASE_THREADS), 0, s, src, ref, dst, n, block, nfull);
    return LAUNCHED();
}

// the ranges [a, a + n) and [b, b + n) are apart (or touch)
bool base_apart(const void* a, const void* b, u64 n)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x >= n : x - y >= n;
}

bool base_args_ok(const rcx_ctx* c, const void* src, const void* ref, u64 n, u32 width, u32 block, u32 op, const void* dst)
{
    if (!c || !(width == 1 || width == 2 || width == 4 || width == 8) || !block_ok(block) || op > RCX_BASE_SUBZZ) return false;
    if (n == 0) return true;
    if (!src || !ref || !dst) return false;
    return base_apart(src, dst, n) && base_apart(ref, dst, n); // (source and base are only read: they may overlap)
}

template <bool JOIN>
int base_device(rcx_ctx* c, const void* d_src, const void* d_base, u64 n, u32 width, u32 block, u32 op, void* d_dst, void* stream)
{
    if (!base_args_ok(c, d_src, d_base, n, width, block, op, d_dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return base_launch<JOIN>(c, static_cast<const u8*>(d_src), static_cast<const u8*>(d_base), n, width, block, op, static_cast<u8*>(d_dst),
                             static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int base_host(rcx_ctx* c, const uint8_t* src, const uint8_t* ref, u64 n, u32 width, u32 block, u32 op, uint8_t* dst)
{
    if (!base_args_ok(c, src, ref, n, width, block, op, dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const u64 ref_at = (n + 15) & ~(u64)15;
    const int r = reserve_staging(c, ref_at + n, n, 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->h_in + ref_at, ref, n, hipMemcpyHostToDevice));
    const int launched = base_launch<JOIN>(c, c->h_in, c->h_in + ref_at, n, width, block, op, c->h_out, nullptr);
    if (launched != RCX_OK) return launched;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_base_split_device(rcx_ctx* c, const void* d_src, const void* d_base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, void* d_dst, void* stream)
{
    return base_device<false>(c, d_src, d_base, n, width, block, op, d_dst, stream);
}

int rcx_base_join_device(rcx_ctx* c, const void* d_src, const void* d_base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, void* d_dst, void* stream)
{
    return base_device<true>(c, d_src, d_base, n, width, block, op, d_dst, stream);
}

int rcx_base_split(rcx_ctx* c, const uint8_t* src, const uint8_t* base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, uint8_t* dst)
{
    return base_host<false>(c, src, base, n, width, block, op, dst);
}

int rcx_base_join(rcx_ctx* c, const uint8_t* src, const uint8_t* base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, uint8_t* dst)
{
    return base_host<true>(c, src, base, n, width, block, op, dst);
}

} // extern "C"
