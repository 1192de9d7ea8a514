/*
 * rcx_predict.h -- a delta predictor for typed integers, in front of the byte-plane filter of rcx_planes.h (new; the
 * reference has no such stage, so the C++ facades get nothing).
 *
 * The plane filter helps floats and small unsorted integers.  Integers that are large in value but small in their
 * differences -- sorted keys, CSR row offsets, positions, timestamps, counters, sampled signals -- keep low byte planes
 * that are close to uniform, and an order-0 coder gets almost nothing out of them.  Their differences are small: the
 * predictor replaces every element by its difference to the element in front, and the planes of the differences code
 * well.  Unsorted data gets WORSE by it, so it is opt-in and never chosen for the caller.
 *
 * The transform.  width = w in {2, 4, 8}, block = B and superblocks of w * B bytes are exactly as in rcx_planes.h.
 * pred = RCX_PRED_NONE (0), RCX_PRED_DELTA (1) or RCX_PRED_ZIGZAG (2).  Elements are little-endian unsigned integers of
 * w bytes; all arithmetic is modulo 2^(8w).  For superblock s with its m whole elements e_0 .. e_(m-1):
 *     delta      d_0 = e_0, d_k = e_k - e_(k-1): the predictor restarts in every superblock
 *     zigzag     additionally every d, d_0 included, becomes z = (d << 1) XOR (0 - (d >> (8w - 1))), logical shifts, so
 *                that small negative differences become small numbers; its inverse is d = (z >> 1) XOR (0 - (z & 1))
 *     the R % w tail bytes keep their values and places
 * and the result goes through the plane split of rcx_planes.h unchanged.  Join with a predictor is the exact inverse:
 * join, un-zigzag, inclusive prefix sum per superblock.  Because the predictor restarts at every superblock border, the
 * transform of a span that starts on a superblock border and ends on one, or at n, is still the transform of that span
 * taken alone.
 *     w = 2, B = 16, bytes 01 00 03 00 06 00 FF FF 02 00 AA   (the elements 1, 3, 6, 65535, 2 and one tail byte)
 *     differences 1, 2, 3, 0xFFF9, 3    delta:   01 02 03 F9 03 00 00 00 FF 00 AA
 *     zigzag      2, 4, 6, 13, 6        zigzag:  02 04 06 0D 06 00 00 00 00 00 AA
 *
 *   rcx_predict_split_device   d_dst = the planes of the predicted d_src
 *   rcx_predict_join_device    d_dst = the elements whose predicted planes d_src holds
 * The contract is that of the rcx_planes_* calls: the device calls only enqueue, on any stream and also under graph
 * capture; they allocate nothing, need no rcx_ctx_reserve and latch nothing.  They read exactly [d_src, d_src + n) and
 * write exactly [d_dst, d_dst + n); pointers may have any alignment.  RCX_E_ARG, before anything is enqueued: what the
 * plane calls refuse (width, block, a null pointer with n > 0, overlapping ranges) and pred > 2.  n = 0 is RCX_OK and
 * does nothing.  pred = RCX_PRED_NONE runs the plane filter alone, so a caller has one call for all three.
 * The host-buffer variants copy in, run the kernel, synchronise and copy out.
 *
 * Join walks a superblock as one chain, a wave to a superblock: it is made for many superblocks (a GiB in 64 KiB
 * blocks has thousands), and a buffer of a few very large blocks joins slowly.
 *
 * The RCX_CODER_RANS8 caveat of rcx_planes.h applies more often here: the predictor makes more planes of one repeated
 * byte, each of which costs that coder 2 bytes a symbol.
 */
#ifndef RCX_PREDICT_H_
#define RCX_PREDICT_H_

#include "rcx_planes.h"

#define RCX_PRED_NONE 0u
#define RCX_PRED_DELTA 1u
#define RCX_PRED_ZIGZAG 2u

#ifdef __cplusplus
extern "C" {
#endif

int rcx_predict_split_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream);
int rcx_predict_join_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, void* d_dst, void* stream);
int rcx_predict_split(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst);
int rcx_predict_join(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t width, uint32_t block, uint32_t pred, uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* RCX_PREDICT_H_ */
