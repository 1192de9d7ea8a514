// rcx_typed_api.hpp -- the calls of include/rcx_planes.h and include/rcx_predict.h, the typed stage in front of the coders:
// one launch per call, of rcx_planes_k (rcx_planes.hpp), or of rcx_predict_join_k (rcx_predict.hpp) for the inverse with a
// predictor.  The plane calls are the predictor calls with RCX_PRED_NONE.
//
// Nothing of the context is used but its device and compute-unit count: no scratch, no table, no latch, nothing to
// reserve, so the device calls can be captured.  The host-buffer calls go through the staging buffers of the other
// host-buffer calls.
#pragma once

#include "../../include/rcx_predict.h"
#include "rcx_ctx.hpp"
#include "rcx_predict.hpp"

namespace
{

typedef void (*TypedKernel)(const u8*, u8*, u64, u32, u64);

template <u32 W, bool JOIN, u32 PRED>
constexpr TypedKernel typed_kernel()
{
    if constexpr (JOIN && PRED != 0) return rcx_predict_join_k<W, PRED == RCX_PRED_ZIGZAG>;
    else return rcx_planes_k<W, JOIN, PRED>;
}

// The grid of rcx_planes_k: a fixed one, four workgroups (16 waves) to a compute unit, that loops; fewer where there is
// less to do.
dim3 planes_grid(const rcx_ctx* c, u64 n, u32 width, u32 block, u64 nfull)
{
    const u64 rest_last = n - nfull * width * block;
    const u64 units = nfull * (block >> 4) + (rest_last / width >> 4);
    const u64 bytewise = nfull * ((block & 15u) * width) + 17ull * width; // (at most: the last superblock's is below 17 * width)
    const u64 per = (u64)(RCX_PLANES_U4 / width) * RCX_PLANES_THREADS;
    u64 want = (units + per - 1) / per;
    if (want < (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS) want = (bytewise + RCX_PLANES_THREADS - 1) / RCX_PLANES_THREADS;
    const u64 most = 4ull * (u64)c->cus;
    return dim3((u32)(want < most ? want : most));
}

template <bool JOIN>
int typed_launch(rcx_ctx* c, const u8* src, u64 n, u32 width, u32 block, u32 pred, u8* dst, hipStream_t s)
{
    static constexpr TypedKernel table[3][3] = {
        {typed_kernel<2, JOIN, 0>(), typed_kernel<2, JOIN, 1>(), typed_kernel<2, JOIN, 2>()},
        {typed_kernel<4, JOIN, 0>(), typed_kernel<4, JOIN, 1>(), typed_kernel<4, JOIN, 2>()},
        {typed_kernel<8, JOIN, 0>(), typed_kernel<8, JOIN, 1>(), typed_kernel<8, JOIN, 2>()},
    };
    const TypedKernel kernel = table[width == 2 ? 0 : width == 4 ? 1 : 2][pred];
    const u64 super = (u64)width * block, nfull = n / super;
    if (JOIN && pred != RCX_PRED_NONE) {
        // a wave to a superblock; a fixed grid of at most 32 waves a compute unit that loops.  The kernels' registers let 4 to 7
        // waves a SIMD be resident, so part of a full grid waits to be scheduled: no wave waits for another, so that is harmless
        const u64 nsuper = nfull + (n - nfull * super ? 1u : 0u);
        const u64 most = 32ull * (u64)c->cus;
        hipLaunchKernelGGL(kernel, dim3((u32)(nsuper < most ? nsuper : most)), dim3(RCX_PREDICT_TILE_UNITS), 0, s, src, dst, n, block, nfull);
    } else {
        hipLaunchKernelGGL(kernel, planes_grid(c, n, width, block, nfull), dim3(RCX_PLANES_THREADS), 0, s, src, dst, n, block, nfull);
    }
    return LAUNCHED();
}

bool typed_args_ok(const rcx_ctx* c, const void* src, u64 n, u32 width, u32 block, u32 pred, const void* dst)
{
    if (!c || !(width == 2 || width == 4 || width == 8) || !block_ok(block) || pred > RCX_PRED_ZIGZAG) return false;
    if (n == 0) return true;
    if (!src || !dst) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
    return a < b ? b - a >= n : a - b >= n; // the ranges [a, a + n) and [b, b + n) are apart (or touch)
}

template <bool JOIN>
int typed_device(rcx_ctx* c, const void* d_src, u64 n, u32 width, u32 block, u32 pred, void* d_dst, void* stream)
{
    if (!typed_args_ok(c, d_src, n, width, block, pred, d_dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    return typed_launch<JOIN>(c, static_cast<const u8*>(d_src), n, width, block, pred, static_cast<u8*>(d_dst), static_cast<hipStream_t>(stream));
}

template <bool JOIN>
int typed_host(rcx_ctx* c, const uint8_t* src, u64 n, u32 width, u32 block, u32 pred, uint8_t* dst)
{
    if (!typed_args_ok(c, src, n, width, block, pred, dst)) return RCX_E_ARG;
    HIP_TRY(rcx_enter_device(c->device));
    if (n == 0) return RCX_OK;
    const int r = reserve_staging(c, n, n, 0);
    if (r != RCX_OK) return r;
    HIP_TRY(hipMemcpy(c->h_in, src, n, hipMemcpyHostToDevice));
    const int launched = typed_launch<JOIN>(c, c->h_in, n, width, block, pred, c->h_out, nullptr);
    if (launched != RCX_OK) return launched;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(dst, c->h_out, n, hipMemcpyDeviceToHost));
    return RCX_OK;
}

} // namespace

extern "C" {

int rcx_planes_split_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream)
{
    return typed_device<false>(c, d_src, n, width, block, RCX_PRED_NONE, d_dst, stream);
}

int rcx_planes_join_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream)
{
    return typed_device<true>(c, d_src, n, width, block, RCX_PRED_NONE, d_dst, stream);
}

int rcx_planes_split(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst)
{
    return typed_host<false>(c, src, n, width, block, RCX_PRED_NONE, dst);
}

int rcx_planes_join(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst)
{
    return typed_host<true>(c, src, n, width, block, RCX_PRED_NONE, dst);
}

int rcx_predict_split_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream)
{
    return typed_device<false>(c, d_src, n, width, block, pred, d_dst, stream);
}

int rcx_predict_join_device(rcx_ctx* c, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream)
{
    return typed_device<true>(c, d_src, n, width, block, pred, d_dst, stream);
}

int rcx_predict_split(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst)
{
    return typed_host<false>(c, src, n, width, block, pred, dst);
}

int rcx_predict_join(rcx_ctx* c, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst)
{
    return typed_host<true>(c, src, n, width, block, pred, dst);
}

} // extern "C"
