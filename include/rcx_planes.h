/*
 * rcx_planes.h -- the byte-plane filter for typed data, in front of the coders of rcx.h (new; the reference has no
 * such stage, so the C++ facades get nothing).
 *
 * The coders are order-0: one model per block.  In typed data -- bf16 / fp16 / fp32 values, int32 / int64 indices --
 * the bytes of one element have very different statistics, and a model over the interleaved bytes sees their
 * mixture.  The filter takes the elements apart so that every coder block holds one byte position only.
 *
 * The transform.  width = w in {2, 4, 8} bytes per element; block = B, the block size the coder will use afterwards,
 * RCX_MIN_BLOCK .. RCX_MAX_BLOCK; n bytes in, n bytes out.  A superblock is w * B source bytes (B elements).  For
 * superblock s, at = s * w * B, with R = min(w * B, n - at) bytes and m = R / w whole elements:
 *     plane p (0 <= p < w), the bytes src[at + p + k * w], k = 0 .. m - 1, goes to dst[at + p * m .. at + (p + 1) * m)
 *     the R % w bytes behind the last whole element are copied to the same positions, dst[at + m * w .. at + R)
 * In a whole superblock (m = B) coder block s * w + p of the output is exactly plane p, with a model of its own.  In
 * the ragged last superblock the coder's block borders need not fall on plane borders.  Join is the inverse.  The
 * transform of a span that starts on a superblock border and ends on one, or at n, is the transform of that span
 * taken alone.
 *     w = 4, B = 16, bytes 0 .. 9   ->   0 4 1 5 2 6 3 7 8 9
 *
 *   rcx_planes_split_device   d_dst = the planes of d_src
 *   rcx_planes_join_device    d_dst = the elements whose planes d_src holds
 * The device calls only enqueue, on any stream and also under graph capture; they allocate nothing, need no
 * rcx_ctx_reserve and latch nothing (there is nothing that can fail on the device).  They read exactly
 * [d_src, d_src + n) and write exactly [d_dst, d_dst + n); pointers may have any alignment.
 * RCX_E_ARG, before anything is enqueued: a width other than 2, 4 or 8, a block size outside RCX_MIN_BLOCK ..
 * RCX_MAX_BLOCK, a null pointer with n > 0, source and destination ranges that overlap (the transform is not done in
 * place; ranges that only touch are fine).  n = 0 is RCX_OK and does nothing.
 * The host-buffer variants copy in, run the kernel, synchronise and copy out.
 *
 * One thing to know about RCX_CODER_RANS8 behind the filter: a plane of one repeated byte -- the upper bytes of small
 * int64 values -- costs that coder 2 bytes a symbol, the reference's own behaviour for a frequency of 4096 (see
 * rcx_block_bound_for in rcx.h).  The other three coders code such a plane in a few bytes.
 */
#ifndef RCX_PLANES_H_
#define RCX_PLANES_H_

#include "rcx.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_planes_split_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream);
int rcx_planes_join_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t width, uint32_t block, void* d_dst, void* stream);
int rcx_planes_split(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst);
int rcx_planes_join(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* RCX_PLANES_H_ */
