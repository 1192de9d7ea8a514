// rcx_planes_api.hpp -- the calls of include/rcx_planes.h: one launch of rcx_planes_k (rcx_planes.hpp) per call.
//
// Nothing of the context is used but its device and compute-unit count: no scratch, no table, no latch, nothing to
// reserve, so the device calls can be captured.  The host-buffer calls go through the staging buffers of the other
// host-buffer calls.
#pragma once

#include "../../include/rcx_planes.h"
#include "rcx_ctx.hpp"

namespace
{

template <bool JOIN>
int planes_launch(rcx_ctx* c, const u8* src, u64 n, u32 width, u32 block, u8* dst, hipStream_t s)
{
    const u64 super = (u64)width * block, nfull = n / super;
    const u64 rest_last = n - nfull * super;
    const u64 units = nfull * (block >> 4) + (rest_last / width >> 4);
    const u64 bytewise = nfull * ((block & 15u) * width) + 17ull * width; // (at most: the last superblock's is below 17 * width)
    const u64 per = (u64)(RCX_PLANES_U4 / width) * RCX_PLANES_THREADS;
    // a fixed grid, four workgroups (16 waves) to a compute unit, that loops; fewer where there is less to do
    u64 want = (units + per - 1) / per;
    if (want < (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS) want = (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS;
    const u64 most = 4ull * (u64)c->cus;
    const dim3 grid((u32)(want < most ? want : most)), wg(RCX_PLANES_THREADS);
    if (width == 2) hipLaunchKernelGGL((rcx_planes_k<2, JOIN>), grid, wg, 0, s, src, dst, n, block, nfull);
    else if (width == 4) hipLaunchKernelGGL((rcx_planes_k<4, JOIN>), grid, wg, 0, s, src, dst, n, block, nfull);
    else hipLaunchKernelGGL((rcx_planes_k<8, JOIN>), grid, wg, 0, s, src, dst, n, block, nfull);
    return LAUNCHED();
}

bool planes_args_ok(const rcx_ctx* c, const void* src, u64 n, u32 width, u32 block, const void* dst)
{
    if (!c || !(width == 2 || width == 4 || width == 8) || !block_ok(block)) return false;
    if (n == 0) return true;
    if (!src || !dst) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
    return a < b ? b - a >= n : a - b >= n; // the ranges [a, a + n) and [b, b + n) are apart (or touch)
}

template <bool JOIN>
int planes_device(rcx_ctx* c, const void* d_src, u64 n, u32 width, u32 block, void* d_dst, void* stream)
{
    if (!planes_args_ok(c, d_src, n, width, block, d_dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return planes_launch<JOIN>(c, static_cast<const u8*>(d_src), n, width, block, static_cast<u8*>(d_dst), static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int planes_host(rcx_ctx* c, const uint8_t* src, u64 n, u32 width, u32 block, uint8_t* dst)
{
    if (!planes_args_ok(c, src, n, width, block, dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const int r = reserve_staging(c, n, n, 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    const int launched = planes_launch<JOIN>(c, c->h_in, n, width, block, c->h_out, nullptr);
    if (launched != RCX_OK) return launched;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_planes_split_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream)
{
    return planes_device<false>(c, d_src, n, width, block, d_dst, stream);
}

int rcx_planes_join_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream)
{
    return planes_device<true>(c, d_src, n, width, block, d_dst, stream);
}

int rcx_planes_split(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst)
{
    return planes_host<false>(c, src, n, width, block, dst);
}

int rcx_planes_join(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst)
{
    return planes_host<true>(c, src, n, width, block, dst);
}

} // extern "C"
