/*
 * rcx_typed_split_picks.h -- the typed split per item with every table in device memory: where each item's bytes lie, where
 * its split text goes, its length, width and predictor and how many entries are meant are read by the GPU; the call only
 * enqueues and may be captured in a graph (new; the reference has no typed stage).  The mirror of rcx_typed_picks.h.
 *
 * rcx_typed_items_split_device (rcx_typed_items.h) takes its tables from the HOST, plans on the CPU and uploads the plan
 * inside the call.  Here the plan is made by kernels (csrc/rcx_typed_split_picks.hpp), so the split can stand in front of
 * rcx_encode_picks_device (rcx_encode_picks.h) inside one captured graph and be replayed against tables that another kernel
 * rewrites between the replays: split -> encode -> decode -> join has a device-planned form end to end.
 *
 *   rcx_typed_split_picks_device        entry k < *d_count splits d_src[d_src_at[k] .. + d_len[k]) into d_dst[d_dst_at[k] .. + d_len[k])
 *   rcx_typed_split_picks_reserve       the scratch of such calls with at most max_pick entries of at most max_bytes together
 *   rcx_typed_split_picks_scratch_bytes what rcx_ctx_scratch_bytes reports for a fresh context after that reservation
 *   rcx_typed_split_picks               the same on host buffers: copy in, run, synchronise, copy out; every entry meant
 *
 * What an entry means.  Entry k < min(*d_count, max_pick) is one typed item as rcx_typed_items.h defines it: ONE superblock
 * of m = len / width elements with width d_widths[k] (1, 2, 4, 8) and predictor d_preds[k] (RCX_PRED_*; d_preds = NULL:
 * none has one), the predictor starting at 0 in front of the item; plane p of the split text goes to [p * m, (p + 1) * m) of
 * the entry's destination span, the len % width tail bytes keep their places, width 1 is a copy.  Source and destination
 * positions are separate tables: the items lie where an allocator put them and the split text goes packed into a staging
 * buffer.  d_src_at, d_dst_at and d_len have max_pick entries of uint64_t, d_widths and d_preds max_pick bytes, d_count is one
 * uint64_t.  Entries behind the count may hold anything and are not read; entries need no order; an entry of length 0 is not
 * looked at; any alignment; where two outputs overlap, the bytes of the overlap are unspecified.  Nothing outside the valid
 * entries' output ranges is written.  Every output byte is the one rcx_typed_items_split_device writes for the same item.
 *
 * Validation is the device's, and it is rcx_typed_picks.h's, rule for rule (one function, rcx_tpick_validate): a bad entry is
 * skipped and latched with its position, every other entry is split.  For entry k with len > 0, in this order:
 *     width not 1, 2, 4 or 8; predictor above RCX_PRED_ZIGZAG; a predictor with
 *     width 1; len / w + len % w > RCX_MAX_BLOCK                                skipped, RCX_E_CORRUPT at k
 *     d_src_at[k] + len > src_cap or d_dst_at[k] + len > dst_cap (in integers
 *     of any width: no sum wraps)                                               skipped, RCX_E_CAPACITY at k
 * and for the call:
 *     *d_count > max_pick                                  treated as max_pick, RCX_E_CAPACITY at max_pick
 *     the lengths of the entries that passed sum to more than max_bytes
 *                                                          NOTHING is split, RCX_E_CAPACITY at min(*d_count, max_pick)
 * max_bytes is the caller's promise: it makes the scratch a function of (max_pick, max_bytes) alone and sizes the row table
 * before a capture.  The latch is the usual one: rcx_ctx_sync_status returns RCX_E_CORRUPT if anything was corrupt, else
 * RCX_E_CAPACITY, and the lowest position of either.
 *
 * d_kept, which the join's call has no twin for, may be NULL and has max_pick entries of uint64_t, ALL of which are written:
 * d_kept[k] = d_len[k] if entry k was split; 0 if it has length 0, was skipped, lies at or behind the count, or the call split
 * nothing because of the max_bytes rule.  It is the length table of the stage behind the split (rcx_encode_picks_device), which
 * so needs no second copy of the rules above: a skipped entry has no bytes to encode.
 *
 * RCX_E_ARG, before anything is enqueued, is what the host can see: a null pointer (d_preds and d_kept apart), max_pick >
 * 2^31 - 1, max_bytes > 2^42 (the row table has 32-bit indices: max_bytes / 4096 + 24 rows at the most), [d_src, d_src +
 * src_cap) and [d_dst, d_dst + dst_cap) overlapping (touching is fine).  max_pick = 0 is RCX_OK, looks at no pointer but ctx
 * and enqueues nothing.
 *
 * Scratch and graphs.  After rcx_typed_split_picks_reserve a call with the same or smaller max_pick and max_bytes is five
 * kernel launches on `stream` and nothing else -- no allocation, no copy, no memset node -- whose shapes depend on max_pick,
 * max_bytes and the device's compute units alone; it may be captured.  Without a sufficient reservation the call grows the
 * scratch itself, which under capture is the caller's error.  The tables lie in the context's table scratch, the one every
 * device-planned call plans into and the host-planned item calls upload into: it is as large as the largest reservation of
 * any of them, whichever came first, and calls on one context follow one another on one stream.  With
 * T = (max_pick + 255) / 256 tiles and R = max_bytes / 4096 + 24 rows:
 *     rcx_typed_split_picks_scratch_bytes = 400 + 8 * (max_pick + 1) + 16 * max_pick    the head, ufirst, two position tables
 *                                         + 200 * T + 48 * T                            tile sums (13 + 12 words), tile entries
 *                                         + 8 * max_pick + 4 * R + 8                    len, keys, rows, two words
 *                                         rounded up to a multiple of 8
 * (0 for bad arguments or max_pick = 0).
 *
 * The host-buffer call copies [src, src + src_cap) and [dst, dst + dst_cap) to the device, takes every one of the npick
 * entries as meant and the sum of the valid entries' lengths as max_bytes, and returns the latched status; dst comes back
 * as a whole, the good entries written also behind a latched failure, and kept (NULL or npick entries) as the device wrote it.
 */
#ifndef RCX_TYPED_SPLIT_PICKS_H_
#define RCX_TYPED_SPLIT_PICKS_H_

#include "rcx_typed_picks.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_typed_split_picks_reserve(rcx_ctx* ctx, uint64_t max_pick, uint64_t max_bytes);
uint64_t rcx_typed_split_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes);
int rcx_typed_split_picks_device(rcx_ctx* ctx, const void* d_src, uint64_t src_cap, const uint64_t* d_src_at, const uint64_t* d_dst_at,
                                 const uint64_t* d_len, const uint8_t* d_widths, const uint8_t* d_preds, const uint64_t* d_count, uint64_t max_pick,
                                 uint64_t max_bytes, void* d_dst, uint64_t dst_cap, uint64_t* d_kept, void* stream);
int rcx_typed_split_picks(rcx_ctx* ctx, const uint8_t* src, uint64_t src_cap, const uint64_t* src_at, const uint64_t* dst_at, const uint64_t* len,
                          const uint8_t* widths, const uint8_t* preds, uint64_t npick, uint8_t* dst, uint64_t dst_cap, uint64_t* kept);

#ifdef __cplusplus
}
#endif

#endif /* RCX_TYPED_SPLIT_PICKS_H_ */
