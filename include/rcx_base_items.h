/*
 * rcx_base_items.h -- residuals against a base PER ITEM: the stage of rcx_base.h for MANY BUFFERS OF DIFFERING SIZES IN ONE
 * CALL, each with an element width of its own and either a predictor, or a base op against a span of a second buffer, or
 * neither (new; the reference has no such stage, so the C++ facades get nothing).  It is rcx_typed_items.h with one more
 * choice per item, and the stage in front of the item calls of rcx.h for what a user holds as a state dict: tensors that
 * moved a little against the checkpoint before, tensors that are frozen and equal their base, tensors that are new and
 * have none, sorted keys and offsets that want the predictor instead; KV pages coded against one reference page.
 *
 * The transform (normative).  Item i is
 *     len_i bytes at src_offsets[i] .. src_offsets[i + 1]: items are contiguous, exactly those of rcx_typed_items.h
 *     a width w_i in {1, 2, 4, 8}, and with it m_i = len_i / w_i whole elements and r_i = len_i % w_i tail bytes
 *     a predictor p_i in {RCX_PRED_NONE, RCX_PRED_DELTA, RCX_PRED_ZIGZAG}
 *     a base op o_i in {RCX_BASE_XOR, RCX_BASE_SUB, RCX_BASE_SUBZZ, RCX_BASE_NONE}; an item has a predictor or an op, never both
 *     with an op, a base span: the len_i bytes at base_offsets[i] of the base buffer
 * o_i == RCX_BASE_NONE: the item's transform is that of rcx_typed_items.h, and base_offsets[i] is not looked at.
 * Otherwise it is that of ONE SUPERBLOCK of rcx_base.h with m = m_i against the base span: every whole element e_k becomes
 * its residual against the element b_k at the same place of the span (xor: e_k XOR b_k; sub: e_k - b_k; subzz:
 * z(e_k - b_k); little-endian, modulo 2^(8w), rcx_base.h has the arithmetic), plane p of the residuals goes to
 * [p * m_i, (p + 1) * m_i) of the item's span, and the r_i tail bytes keep the SOURCE's values and places (the span's tail
 * bytes are not looked at).  Width 1 has no planes and is the residual alone.  Join is the exact inverse with the same
 * base.  n bytes in, n bytes out, every item stays in its own span.
 * Base spans are independent of the source's layout: in any order, overlapping, or one span for many items.
 *     item 0   w = 2, subzz, 7 bytes    05 01 00 01 42 00 AA           (rcx_base.h's example)
 *     item 1   w = 2, delta, 11 bytes   01 00 03 00 06 00 FF FF 02 00 AA   (rcx_typed_items.h's), no base
 *     base     EE EE 00 01 02 01 42 00 55, base_offsets = {2, anything}: item 0's span is 00 01 02 01 42 00 55
 *     split    0A 03 00 00 00 00 AA   01 02 03 F9 03 00 00 00 FF 00 AA
 *     with xor item 0 gives 05 02 00 00 00 00 AA, with sub 05 FE 00 00 FF 00 AA
 *
 * On common ground it is the existing calls, byte for byte:
 *   ops == NULL means no item has an op; d_base and base_offsets may then be NULL, and the calls write what
 *     rcx_typed_items_split_device / rcx_typed_items_join_device write;
 *   a buffer cut into items of w * B bytes, its ragged rest as the last item, all with one width and one op and no
 *     predictor, base_offsets == src_offsets: the calls write what rcx_base_split_device(n, w, B, op) writes.
 *
 * The coder's items behind it are the sub-items of rcx_typed_items.h: rcx_typed_items_sub_count and
 * rcx_typed_items_sub_offsets serve this stage as they are.
 *
 *   rcx_base_items_split_device   d_dst = the transform of every item of d_src
 *   rcx_base_items_join_device    the inverse
 *   rcx_base_items_split, _join   the same on host buffers: copy items and the base spans in use in, run, synchronise,
 *                                 copy out; base_bytes = the size of `base`
 *   rcx_base_items_check          RCX_OK or RCX_E_ARG: what the calls refuse in the tables alone
 *   rcx_base_items_hull           the same, and [*lo, *hi) = the hull of the base spans in use (0, 0 where there is none)
 * The last two are pure functions of their arguments.
 *
 * The contract is rcx_typed_items.h's.  src_offsets (nitems + 1 entries), base_offsets (nitems entries), widths, preds and
 * ops (nitems bytes each; preds == NULL: no predictor, ops == NULL: no op) are HOST tables.  The call plans on the host and
 * sends its tables inside the call, in one copy, into the context's scratch (rcx_ctx_scratch_bytes counts them).  SO THE
 * CALLS CANNOT BE CAPTURED INTO A GRAPH; they enqueue on the given stream and return.  A context serves one call at a
 * time, on one stream at a time.  The number of launches does not depend on nitems: at most two for split, at most three
 * for join.  Nothing is latched.  They read exactly [d_src + src_offsets[0], d_src + src_offsets[nitems]) and the whole
 * elements of the base spans in use, and write exactly the source's range of d_dst; the source range, the destination range
 * and every base span may sit at any alignment.
 *
 * RCX_E_ARG, before anything is enqueued or written: everything rcx_typed_items.h refuses; an op other than 0, 1, 2 or
 * RCX_BASE_NONE; an item with both a predictor and an op; ops given with base_offsets or d_base NULL while an item with an
 * op has bytes; a base span that wraps around 2^64, or, in the host variants, ends past base_bytes; a destination range
 * that overlaps the source range OR THE HULL OF THE BASE SPANS IN USE -- from the lowest base_offsets[i] to the highest
 * base_offsets[i] + len_i over the items with an op and with bytes: the hull is tested, not each span, so a destination in
 * a gap between two spans is refused.  Ranges that touch count as apart.  Source and base may overlap: both are only read.
 *
 * The residual decodes correctly whatever the base is: a wrong base gives wrong elements and no error.  A container that
 * uses this stage should carry a checksum of every base span (cpprcoder_amd/layout.py, RCXK, does).
 */
#ifndef RCX_BASE_ITEMS_H_
#define RCX_BASE_ITEMS_H_

#include "rcx_base.h"
#include "rcx_typed_items.h"

#define RCX_BASE_NONE 0xFFu

#ifdef __cplusplus
extern "C" {
#endif

int rcx_base_items_check(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                         uint64_t nitems);
int rcx_base_items_hull(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                        uint64_t nitems, uint64_t* lo, uint64_t* hi);

int rcx_base_items_split_device(rcx_ctx* ctx, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                                const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, void* d_dst, void* stream);
int rcx_base_items_join_device(rcx_ctx* ctx, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                               const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, void* d_dst, void* stream);
int rcx_base_items_split(rcx_ctx* ctx, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets,
                         const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, uint8_t* dst);
int rcx_base_items_join(rcx_ctx* ctx, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets,
                        const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops, uint64_t nitems, uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* RCX_BASE_ITEMS_H_ */
