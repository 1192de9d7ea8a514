// rcx_predict_api.hpp -- the calls of include/rcx_predict.h: one launch per call, of rcx_predict_split_k / rcx_predict_join_k
// (rcx_predict.hpp), or of rcx_planes_k when no predictor is asked for.
//
// As with the plane calls, nothing of the context is used but its device and compute-unit count: no scratch, no table, no
// latch, nothing to reserve, so the device calls can be captured.  The argument checks are those of the plane calls
// (planes_args_ok) and pred <= 2.
#pragma once

#include "../../include/rcx_predict.h"
#include "rcx_planes_api.hpp"
#include "rcx_predict.hpp"

namespace
{

template <bool ZIGZAG>
int predict_split_launch(rcx_ctx* c, const u8* src, u64 n, u32 width, u32 block, u8* dst, hipStream_t s)
{
    // the grid of planes_launch: the kernel has its shape
    const u64 super = (u64)width * block, nfull = n / super;
    const u64 rest_last = n - nfull * super;
    const u64 units = nfull * (block >> 4) + (rest_last / width >> 4);
    const u64 bytewise = nfull * ((block & 15u) * width) + 17ull * width;
    const u64 per = (u64)(RCX_PLANES_U4 / width) * RCX_PLANES_THREADS;
    u64 want = (units + per - 1) / per;
    if (want < (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS) want = (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS;
    const u64 most = 4ull * (u64)c->cus;
    const dim3 grid((u32)(want < most ? want : most)), wg(RCX_PLANES_THREADS);
    if (width == 2) hipLaunchKernelGGL((rcx_predict_split_k<2, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    else if (width == 4) hipLaunchKernelGGL((rcx_predict_split_k<4, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    else hipLaunchKernelGGL((rcx_predict_split_k<8, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    return LAUNCHED();
}

template <bool ZIGZAG>
int predict_join_launch(rcx_ctx* c, const u8* src, u64 n, u32 width, u32 block, u8* dst, hipStream_t s)
{
    // a wave to a superblock; a fixed grid of at most 32 waves a compute unit that loops.  The kernels' registers let 4 to 7
    // waves a SIMD be resident, so part of a full grid waits to be scheduled: no wave waits for another, so that is harmless
    const u64 super = (u64)width * block, nfull = n / super;
    const u64 nsuper = nfull + (n - nfull * super ? 1u : 0u);
    const u64 most = 32ull * (u64)c->cus;
    const dim3 grid((u32)(nsuper < most ? nsuper : most)), wg(RCX_PREDICT_TILE_UNITS);
    if (width == 2) hipLaunchKernelGGL((rcx_predict_join_k<2, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    else if (width == 4) hipLaunchKernelGGL((rcx_predict_join_k<4, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    else hipLaunchKernelGGL((rcx_predict_join_k<8, ZIGZAG>), grid, wg, 0, s, src, dst, n, block, nfull);
    return LAUNCHED();
}

template <bool JOIN>
int predict_launch(rcx_ctx* c, const u8* src, u64 n, u32 width, u32 block, u32 pred, u8* dst, hipStream_t s)
{
    if (pred == RCX_PRED_NONE) return planes_launch<JOIN>(c, src, n, width, block, dst, s);
    if (JOIN) return pred == RCX_PRED_ZIGZAG ? predict_join_launch<true>(c, src, n, width, block, dst, s) : predict_join_launch<false>(c, src, n, width, block, dst, s);
    return pred == RCX_PRED_ZIGZAG ? predict_split_launch<true>(c, src, n, width, block, dst, s) : predict_split_launch<false>(c, src, n, width, block, dst, s);
}

template <bool JOIN>
int predict_device(rcx_ctx* c, const void* d_src, u64 n, u32 width, u32 block, u32 pred, void* d_dst, void* stream)
{
    if (pred > RCX_PRED_ZIGZAG || !planes_args_ok(c, d_src, n, width, block, d_dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return predict_launch<JOIN>(c, static_cast<const u8*>(d_src), n, width, block, pred, static_cast<u8*>(d_dst), static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int predict_host(rcx_ctx* c, const uint8_t* src, u64 n, u32 width, u32 block, u32 pred, uint8_t* dst)
{
    if (pred > RCX_PRED_ZIGZAG || !planes_args_ok(c, src, n, width, block, dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const int r = reserve_staging(c, n, n, 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    const int launched = predict_launch<JOIN>(c, c->h_in, n, width, block, pred, c->h_out, nullptr);
    if (launched != RCX_OK) return launched;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_predict_split_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream)
{
    return predict_device<false>(c, d_src, n, width, block, pred, d_dst, stream);
}

int rcx_predict_join_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream)
{
    return predict_device<true>(c, d_src, n, width, block, pred, d_dst, stream);
}

int rcx_predict_split(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst)
{
    return predict_host<false>(c, src, n, width, block, pred, dst);
}

int rcx_predict_join(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst)
{
    return predict_host<true>(c, src, n, width, block, pred, dst);
}

} // extern "C"
