/*
 * rcx_base.h -- residuals against a base buffer, in front of the byte-plane filter of rcx_planes.h (new; the reference has
 * no such stage, so the C++ facades get nothing).
 *
 * Typed buffers often differ a little from one the reader already has: a checkpoint against the one before it, a
 * fine-tuned model against its base model, a KV page or a counter table against its last snapshot.  The plane filter sees
 * only the new buffer, and the delta predictor of rcx_predict.h looks at the neighbouring element, which says nothing
 * about a weight.  This stage replaces every element by its residual against the element at the same place of the BASE,
 * a second buffer of the same length that the reader must hold as well, and the planes of the residuals code well.
 * Against an unrelated base the data gets WORSE by it, so it is opt-in and never chosen for the caller.
 *
 * The transform.  width = w in {1, 2, 4, 8} bytes per element; block = B, RCX_MIN_BLOCK .. RCX_MAX_BLOCK; n bytes of the
 * source, n bytes of the base, n bytes out.  For w = 2, 4, 8 the superblocks of w * B bytes, their m whole elements, the
 * planes and the R % w tail bytes are exactly those of rcx_planes.h.  Width 1 (fp8 and byte tensors) has no planes: a
 * superblock is one block and the split is the residual alone.  op = RCX_BASE_XOR (0), RCX_BASE_SUB (1) or
 * RCX_BASE_SUBZZ (2).  Elements are little-endian unsigned integers of w bytes; all arithmetic is modulo 2^(8w).  For every
 * whole element e_k of a superblock and the base's element b_k at the same place:
 *     xor        r_k = e_k XOR b_k
 *     sub        r_k = e_k - b_k
 *     subzz      r_k = z(e_k - b_k), z(d) = (d << 1) XOR (0 - (d >> (8w - 1))), logical shifts: the zigzag of
 *                rcx_predict.h, so that small differences of both signs become small numbers
 *     the R % w tail bytes keep the SOURCE's values and places (the base's tail bytes are not looked at)
 * and the residuals go through the plane split of rcx_planes.h unchanged.  Join is the exact inverse, with the same base:
 * the planes put together, then e_k = r_k XOR b_k, r_k + b_k, or z^-1(r_k) + b_k.  The transform is elementwise -- no
 * element depends on another -- so the transform of a span that starts on a superblock border and ends on one, or at n,
 * is the transform of that span AND THE SAME SPAN OF THE BASE taken alone.
 *     w = 2, B = 16, source 05 01 00 01 42 00 AA   (the elements 0x0105, 0x0100, 0x0042 and one tail byte)
 *                    base   00 01 02 01 42 00 55   (the elements 0x0100, 0x0102, 0x0042: below, above, equal)
 *     residuals  xor 5, 2, 0          split:  05 02 00 00 00 00 AA
 *                sub 5, 0xFFFE, 0     split:  05 FE 00 00 FF 00 AA
 *              subzz 10, 3, 0         split:  0A 03 00 00 00 00 AA
 *
 *   rcx_base_split_device   d_dst = the planes of the residuals of d_src against d_base
 *   rcx_base_join_device    d_dst = the elements whose residuals' planes d_src holds, against the same d_base
 * The contract is that of the rcx_planes_* calls: the device calls only enqueue, on any stream and also under graph
 * capture; they allocate nothing, need no rcx_ctx_reserve and latch nothing.  They read exactly [d_src, d_src + n) and
 * [d_base, d_base + n) and write exactly [d_dst, d_dst + n); all three pointers may have any alignment.
 * RCX_E_ARG, before anything is enqueued: a width other than 1, 2, 4 or 8, a block size outside RCX_MIN_BLOCK ..
 * RCX_MAX_BLOCK, op > 2 (also with n = 0), a null pointer with n > 0, a destination range that overlaps the source's or
 * the base's (ranges that only touch are apart).  Source and base may overlap or be the same: both are only read.
 * n = 0 is RCX_OK and does nothing.
 * The host-buffer variants copy source and base in, run the kernel, synchronise and copy out, through the context's
 * staging buffers (which then hold 2n bytes of input).
 *
 * The residual decodes correctly whatever the base is: a wrong base gives wrong elements and no error.  A container that
 * uses this stage should carry a checksum of the base (cpprcoder_amd/layout.py, RCXD, does).
 */
#ifndef RCX_BASE_H_
#define RCX_BASE_H_

#include "rcx_planes.h"

#define RCX_BASE_XOR 0u
#define RCX_BASE_SUB 1u
#define RCX_BASE_SUBZZ 2u

#ifdef __cplusplus
extern "C" {
#endif

int rcx_base_split_device(rcx_ctx* ctx, const void* d_src, const void* d_base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, void* d_dst, void* stream);
int rcx_base_join_device(rcx_ctx* ctx, const void* d_src, const void* d_base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, void* d_dst, void* stream);
int rcx_base_split(rcx_ctx* ctx, const uint8_t* src, const uint8_t* base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, uint8_t* dst);
int rcx_base_join(rcx_ctx* ctx, const uint8_t* src, const uint8_t* base, uint64_t n, uint32_t width, uint32_t block, uint32_t op, uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* RCX_BASE_H_ */
