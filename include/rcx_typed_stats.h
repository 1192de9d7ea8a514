/*
 * rcx_typed_stats.h -- the order-0 cost of EVERY CANDIDATE TRANSFORM of every item, in one pass over source and base (new;
 * the reference has no such call, so the C++ facades get nothing).
 *
 * An item of rcx_base_items.h can be coded as it is, behind a predictor of rcx_predict.h, or as a residual against its base
 * span under one of the three ops of rcx_base.h.  Which of the six is cheapest depends on the data -- a tensor that moved a
 * little wants subzz, a tensor with a few flipped bits xor, sorted keys delta, a re-initialised tensor no base at all -- and
 * finding out with the existing calls is six splits (rcx_base_items_split_device) and six cost passes
 * (rcx_stats_items_device): twelve reads and six writes of the data for six numbers per item.  These calls read source and
 * base once, form the residuals of all asked candidates in registers and count them.
 *
 * Candidates.  A candidate is the predictor's number, or 3 + the base op's number:
 *     RCX_CAND_NONE 0   RCX_CAND_DELTA 1   RCX_CAND_ZIGZAG 2   RCX_CAND_XOR 3   RCX_CAND_SUB 4   RCX_CAND_SUBZZ 5
 * masks[i] (HOST table, nitems bytes): bit c asks for candidate c of item i.
 *
 * cost[6 * i + c] (normative), for an asked candidate: take item i as rcx_base_items_split would write it with that
 * predictor or op; cut the result at the sub-item borders of rcx_typed_items_sub_offsets -- w planes of m = len / w bytes,
 * the last one with the r = len % w tail bytes, which keep the source's values -- and sum the `cost` of rcx_stats.h over
 * those w sub-items.  The cost of a candidate that was not asked for is 0, so the whole table of 6 * nitems words is defined
 * behind the call.  Integers only: the table equals the composition of the two existing calls exactly, on every machine.
 *     item 0   w = 2, 7 bytes    05 01 00 01 42 00 AA      base span 00 01 02 01 42 00 55      (rcx_base_items.h's example)
 *       none    05 00 42 | 01 01 00 AA     planes of 3 and 3 + 1 bytes: 3 L(3) + (4 L(4) - 2 L(2))          = 311616 + 393216
 *       subzz   0A 03 00 | 00 00 00 AA     3 L(3) + (4 L(4) - 3 L(3))                                       = 311616 + 212672
 *       xor     05 02 00 | 00 00 00 AA     the same counts as subzz
 *       sub     05 FE 00 | 00 FF 00 AA     3 L(3) + (4 L(4) - 2 L(2))                                       = 311616 + 393216
 *     item 1   w = 2, 11 bytes   01 00 03 00 06 00 FF FF 02 00 AA
 *       delta   01 02 03 F9 03 | 00 00 00 FF 00 AA     5 L(5) - 2 L(2) + (6 L(6) - 4 L(4))
 *
 *   rcx_typed_stats_items_device   the table of the items of d_src against d_base
 *   rcx_typed_stats_items          the same on host buffers: copy items and the base spans in use in, run, synchronise, copy
 *                                  the table out; base_bytes = the size of `base`
 *   rcx_typed_stats_check          RCX_OK or RCX_E_ARG: what the calls refuse in the tables alone; a pure function
 *
 * Items, widths, base spans, host tables and alignment rules are exactly those of rcx_base_items.h.  The call plans on the
 * host and sends its tables inside the call, in one copy, into the context's scratch (rcx_ctx_scratch_bytes counts them):
 * it cannot be captured into a graph.  It enqueues on the given stream and returns; nothing is latched.  The number of
 * launches does not depend on nitems: at most four, one per width in use.  It reads exactly the items' bytes and the whole
 * elements of the base spans of the items that ask for an op candidate, and writes exactly 6 * nitems words of d_cost
 * (8-byte aligned).
 *
 * RCX_E_ARG, before anything is enqueued or written: everything rcx_base_items_check refuses in the shared tables
 * (offsets, widths, item lengths, nitems); masks NULL; a mask bit at or above 6; a predictor bit on a width-1 item; an op
 * bit while d_base or base_offsets is NULL and the item has bytes; a base span that wraps around 2^64, or, in the host
 * variant, ends past base_bytes; d_cost NULL, misaligned, or overlapping the source range or the hull of the base spans in
 * use (of the items with an op bit and with bytes).  nitems == 0 is RCX_OK and does nothing; all masks 0 is RCX_OK and zeroes
 * the table.
 */
#ifndef RCX_TYPED_STATS_H_
#define RCX_TYPED_STATS_H_

#include "rcx_base_items.h"
#include "rcx_stats.h"

#define RCX_CAND_NONE 0
#define RCX_CAND_DELTA 1
#define RCX_CAND_ZIGZAG 2
#define RCX_CAND_XOR 3
#define RCX_CAND_SUB 4
#define RCX_CAND_SUBZZ 5
#define RCX_CANDS 6

#ifdef __cplusplus
extern "C" {
#endif

int rcx_typed_stats_check(const uint64_t* src_offsets, const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* masks, uint64_t nitems);
int rcx_typed_stats_items_device(rcx_ctx* ctx, const void* d_src, const void* d_base, const uint64_t* src_offsets, const uint64_t* base_offsets,
                                 const uint8_t* widths, const uint8_t* masks, uint64_t nitems, uint64_t* d_cost, void* stream);
int rcx_typed_stats_items(rcx_ctx* ctx, const uint8_t* src, const uint8_t* base, uint64_t base_bytes, const uint64_t* src_offsets,
                          const uint64_t* base_offsets, const uint8_t* widths, const uint8_t* masks, uint64_t nitems, uint64_t* cost);

#ifdef __cplusplus
}
#endif

#endif /* RCX_TYPED_STATS_H_ */
