/*
 * rcx_typed_items.h -- the typed stage per item: the byte-plane filter of rcx_planes.h and the predictor of rcx_predict.h
 * for MANY BUFFERS OF DIFFERING SIZES IN ONE CALL, each with an element width and a predictor of its own (new; the
 * reference has no such stage, so the C++ facades get nothing).  It is the stage in front of the item calls of rcx.h
 * (rcx_encode_items* / rcx_decode_items*), as rcx_predict_split* is the stage in front of the block calls: the tensors of
 * a state dict, KV-cache pages, gradient buckets, batches of records.
 *
 * The transform (normative).  A typed item i is
 *     len_i bytes at src_offsets[i] .. src_offsets[i + 1]: items are contiguous, as in the item calls
 *     a width w_i in {1, 2, 4, 8}
 *     a predictor p_i in {RCX_PRED_NONE, RCX_PRED_DELTA, RCX_PRED_ZIGZAG}
 * and with them m_i = len_i / w_i whole elements and r_i = len_i % w_i tail bytes.  Its transform is that of ONE
 * SUPERBLOCK of rcx_planes.h / rcx_predict.h with m = m_i: the predictor starts at 0 in front of the item's first element
 * (all arithmetic modulo 2^(8w)), plane p goes to [p * m_i, (p + 1) * m_i) of the item's span, and the r_i tail bytes
 * keep their values and places.  Width 1 takes RCX_PRED_NONE only and is a copy.  n bytes in, n bytes out, every item
 * stays in its own span.
 *     w = 2, delta, the 11 bytes 01 00 03 00 06 00 FF FF 02 00 AA  ->  01 02 03 F9 03 00 00 00 FF 00 AA   (rcx_predict.h)
 *
 * On common ground it is the existing calls: a buffer cut into items of w * B bytes, its ragged rest as the last item,
 * all with one width and predictor, transforms byte for byte to what rcx_predict_split_device(n, w, B, pred) writes.
 *
 * The coder's items behind it are the SUB-ITEMS: typed item i gives w_i of them, its planes in order, each m_i bytes
 * long, the last m_i + r_i.  Sub-items of length 0 are allowed and have no stream, as in the item calls.
 * m_i + r_i <= RCX_MAX_BLOCK, else RCX_E_ARG.
 *   rcx_typed_items_sub_count    the number of sub-items: the sum of the widths (0 if one of them is not 1, 2, 4 or 8)
 *   rcx_typed_items_sub_offsets  their table, sub_count + 1 entries beginning with src_offsets[0] (0 where nitems = 0 and
 *                                src_offsets is NULL): the src_offsets that
 *                                rcx_encode_items_device, rcx_stats_items_device and rcx_crc32_items_device take behind a
 *                                split, and the dst_offsets of rcx_decode_items_device in front of a join
 * Both are pure functions of their arguments.
 *
 *   rcx_typed_items_split_device   d_dst = the transform of every item of d_src
 *   rcx_typed_items_join_device    the inverse
 * src_offsets (nitems + 1 entries), widths and preds (nitems bytes each; preds == NULL: no item has a predictor) are HOST
 * tables.  The call plans on the host -- items by (width, predictor), their units of 16 elements numbered through, for
 * join the items with a predictor longest first -- and sends its tables inside the call, into the context's scratch
 * (rcx_ctx_scratch_bytes counts them).  SO THE CALLS CANNOT BE CAPTURED INTO A GRAPH, as the item calls cannot (the join
 * that can is rcx_typed_join_picks_device of rcx_typed_picks.h, which reads its tables on the device); they
 * enqueue on the given stream and return.  A context serves one call at a time, on one stream at a time.  The number of
 * launches does not depend on nitems: one for split, at most two for join.
 * They read exactly [d_src + src_offsets[0], d_src + src_offsets[nitems]) and write exactly the same range of d_dst, at
 * any alignment of the pointers and of every item.  Nothing is latched.
 *
 * RCX_E_ARG, before anything is enqueued or written: a width outside 1, 2, 4, 8; a predictor above RCX_PRED_ZIGZAG, or any
 * predictor with width 1; decreasing offsets; a sub-item above RCX_MAX_BLOCK; a null table with nitems > 0; a null pointer
 * with bytes to move; source and destination ranges that overlap (touching is fine).  nitems = 0, or no bytes at all, is
 * RCX_OK and does nothing.
 * The host-buffer variants copy in, run, synchronise and copy out.
 *
 * Join with a predictor walks an item as one chain, a wave to an item: made for many items, and an item of many MiB joins
 * slowly, as a large superblock does in rcx_predict.h.
 */
#ifndef RCX_TYPED_ITEMS_H_
#define RCX_TYPED_ITEMS_H_

#include "rcx_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

uint64_t rcx_typed_items_sub_count(const uint8_t* widths, uint64_t nitems);
int rcx_typed_items_sub_offsets(const uint64_t* src_offsets, const uint8_t* widths, uint64_t nitems, uint64_t* sub_offsets);

int rcx_typed_items_split_device(rcx_ctx* ctx, const void* d_src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds,
                                 uint64_t nitems, void* d_dst, void* stream);
int rcx_typed_items_join_device(rcx_ctx* ctx, const void* d_src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds,
                                uint64_t nitems, void* d_dst, void* stream);
int rcx_typed_items_split(rcx_ctx* ctx, const uint8_t* src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                          uint8_t* dst);
int rcx_typed_items_join(rcx_ctx* ctx, const uint8_t* src, const uint64_t* src_offsets, const uint8_t* widths, const uint8_t* preds, uint64_t nitems,
                         uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* RCX_TYPED_ITEMS_H_ */
