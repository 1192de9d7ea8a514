/*
 * rcx_base_picks.h -- the join per item of rcx_base_items.h with every table in device memory: where each item's split text
 * lies, where its base span lies, where its joined bytes go, its length, width, predictor and base op and how many entries
 * are meant are read by the GPU; the call only enqueues and may be captured in a graph (new; the reference has no such
 * stage).
 *
 * rcx_base_items_join_device (rcx_base_items.h) takes its tables from the HOST, plans on the CPU and uploads the plan inside
 * the call.  Here the plan is made by kernels (csrc/rcx_base_picks.hpp), so the join can follow rcx_decode_picks_device
 * (rcx_picks.h) inside one captured graph and be replayed against tables that another kernel rewrites between the replays:
 * rcx_typed_picks.h with one more choice per entry, an op against a base span.
 *
 *   rcx_base_join_picks_device    entry k < *d_count joins d_src[d_src_at[k] .. + d_len[k]) into d_dst[d_dst_at[k] .. + d_len[k]),
 *                                 with an op against d_base[d_base_at[k] .. + d_len[k])
 *   rcx_base_picks_reserve        the scratch of such calls with at most max_pick entries of at most max_bytes together
 *   rcx_base_picks_scratch_bytes  what rcx_ctx_scratch_bytes reports for a fresh context after that reservation
 *   rcx_base_join_picks           the same on host buffers: copy in, run, synchronise, copy out; every entry meant
 *
 * What an entry means.  Entry k < min(*d_count, max_pick) is one item as rcx_base_items.h defines it.  Its split text lies at
 * d_src[d_src_at[k] .. + len) and its joined bytes go to d_dst[d_dst_at[k] .. + len), len = d_len[k], with width d_widths[k]
 * (1, 2, 4, 8), predictor d_preds[k] (RCX_PRED_*) and op d_ops[k]:
 *     d_ops[k] == RCX_BASE_NONE                  a typed item, exactly the entry of rcx_typed_picks.h; d_base_at[k] is not read
 *     RCX_BASE_XOR, RCX_BASE_SUB, RCX_BASE_SUBZZ joined against the span d_base[d_base_at[k] .. + len): only the whole elements
 *                                                of the span are read, the len % width tail bytes keep the source's values
 * Base spans may repeat, overlap and stand in any order: one span for a thousand pages is the KV case.  d_src_at, d_base_at,
 * d_dst_at and d_len have max_pick entries of uint64_t, d_widths, d_preds and d_ops max_pick bytes, d_count is one uint64_t.
 * Entries behind the count may hold anything and are never read; entries need no order; an entry of length 0 is not looked
 * at; any alignment of all three buffers; where two outputs overlap, the bytes of the overlap are unspecified.  Nothing
 * outside the valid entries' output ranges is written.
 *
 * Validation is the device's, as in rcx_typed_picks.h: a bad entry is skipped and latched with its position, every other
 * entry joins.  For entry k with len > 0, in this order:
 *   1. skipped, RCX_E_CORRUPT at k:
 *        width not 1, 2, 4 or 8; predictor above RCX_PRED_ZIGZAG; a predictor with width 1;
 *        op not 0, 1, 2 or RCX_BASE_NONE; a predictor and an op together; len / w + len % w > RCX_MAX_BLOCK
 *   2. skipped, RCX_E_CAPACITY at k (in integers of any width: no sum wraps):
 *        d_src_at[k] + len > src_cap; d_dst_at[k] + len > dst_cap; with an op, d_base_at[k] + len > base_cap
 * and for the call:
 *     *d_count > max_pick                                  treated as max_pick, RCX_E_CAPACITY at max_pick
 *     the lengths of the entries that passed sum to more than max_bytes
 *                                                          NOTHING is joined, RCX_E_CAPACITY at min(*d_count, max_pick)
 * max_bytes is the caller's promise: it makes the scratch a function of (max_pick, max_bytes) alone and sizes both row tables
 * before a capture.  The latch is the usual one: rcx_ctx_sync_status returns RCX_E_CORRUPT if anything was corrupt, else
 * RCX_E_CAPACITY, and the lowest position of either.
 *
 * RCX_E_ARG, before anything is enqueued, is what the host can see: a null pointer -- d_preds may be NULL (no entry has a
 * predictor), d_ops may be NULL (no entry has an op), and then d_base and d_base_at may be NULL too; d_ops given with d_base
 * or d_base_at NULL while base_cap > 0; max_pick > 2^31 - 1; max_bytes > 2^42 (the row tables have 32-bit indices);
 * [d_dst, d_dst + dst_cap) overlapping [d_src, d_src + src_cap) or, with d_ops, [d_base, d_base + base_cap) (touching is
 * fine; source and base may overlap: both are only read).  max_pick = 0 is RCX_OK, looks at no pointer but ctx and enqueues
 * nothing.
 *
 * Common ground: with d_ops == NULL the call writes and latches exactly what rcx_typed_join_picks_device does for the same
 * tables; d_base, base_cap and d_base_at are then not looked at.
 *
 * Scratch and graphs.  After rcx_base_picks_reserve a call with the same or smaller max_pick and max_bytes is NINE kernel
 * launches on `stream` at the most and nothing else -- six of the planner, then the typed set's rows, the typed set's scan
 * list (not with d_preds == NULL) and the base set's rows (not with d_ops == NULL) -- no allocation, no copy, no memset
 * node, one after the other as a chain without parallel branches; their shapes depend on max_pick, max_bytes and the device's
 * compute units alone; it may be captured.  A kernel whose set is empty on the device is launched all the same and finds
 * nothing to do.  Without a sufficient reservation the call grows the scratch itself, which under capture is the caller's
 * error.  The tables lie in the context's table scratch, the one rcx_decode_picks_device and rcx_typed_join_picks_device
 * plan into and the host-planned item calls upload into: it is as large as the largest reservation of any of them, whichever
 * came first, and calls on one context follow one another on one stream.  With T = (max_pick + 255) / 256 tiles,
 * R = max_bytes / 4096 + 8 rows of the typed set and Rb = max_bytes / 4096 + 24 rows of the base set (a unit has 16 bytes
 * at least, a row 256 units, and each of its 12 classes one more row than whole ones and one closing entry):
 *     rcx_base_picks_scratch_bytes = 800 + 16 * (max_pick + 1) + 56 * max_pick + 264 * T       two heads, two ufirst, seven position tables, tile sums
 *                                  + 64 * T + 16 * max_pick + 4 * (R + Rb) + 8 * 5120 + 8      tile entries, len, blen, scan_len, keys, rows, bins, two words
 *                                  + max_pick, rounded up to a multiple of 8                   the scan list's kinds
 * (0 for bad arguments or max_pick = 0).
 *
 * The host-buffer call copies [src, src + src_cap), [base, base + base_cap) and [dst, dst + dst_cap) to the device, takes
 * every one of the npick entries as meant and the sum of the valid entries' lengths as max_bytes, and returns the latched
 * status; dst comes back as a whole, the good entries written also behind a latched failure.
 */
#ifndef RCX_BASE_PICKS_H_
#define RCX_BASE_PICKS_H_

#include "rcx_base_items.h"
#include "rcx_typed_picks.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_base_picks_reserve(rcx_ctx* ctx, uint64_t max_pick, uint64_t max_bytes);
uint64_t rcx_base_picks_scratch_bytes(uint64_t max_pick, uint64_t max_bytes);
int rcx_base_join_picks_device(rcx_ctx* ctx, const void* d_src, uint64_t src_cap, const void* d_base, uint64_t base_cap, const uint64_t* d_src_at,
                               const uint64_t* d_base_at, const uint64_t* d_dst_at, const uint64_t* d_len, const uint8_t* d_widths, const uint8_t* d_preds,
                               const uint8_t* d_ops, const uint64_t* d_count, uint64_t max_pick, uint64_t max_bytes, void* d_dst, uint64_t dst_cap, void* stream);
int rcx_base_join_picks(rcx_ctx* ctx, const uint8_t* src, uint64_t src_cap, const uint8_t* base, uint64_t base_cap, const uint64_t* src_at,
                        const uint64_t* base_at, const uint64_t* dst_at, const uint64_t* len, const uint8_t* widths, const uint8_t* preds, const uint8_t* ops,
                        uint64_t npick, uint8_t* dst, uint64_t dst_cap);

#ifdef __cplusplus
}
#endif

#endif /* RCX_BASE_PICKS_H_ */
