/*
 * rcx_encode_picks.h -- item encode with every table in device memory: where the items lie, how long they are and how
 * many are meant are read by the GPU, the call only enqueues, and it may be captured in a graph -- in front of
 * rcx_decode_picks_device (rcx_picks.h) if wanted, with nothing downloaded in between (new; the reference encodes one buffer
 * per call on the CPU, so the C++ facades get nothing).
 *
 * rcx_encode_items_device (rcx.h) takes `src_offsets` from the HOST, plans on the CPU and uploads the plan inside the call.
 * Here the plan is made by kernels (csrc/rcx_encode_picks.hpp), so a captured graph can be replayed against tables that
 * another kernel rewrites between the replays: pages to evict, buckets that changed, rows a filter kept.
 *
 *   rcx_encode_picks_device         entry k < *d_count encodes d_src[d_src_at[k] .. d_src_at[k] + d_src_len[k]) as STREAM k of
 *                                   the set [d_dst, ..) / d_comp_offsets[0 .. max_items]
 *   rcx_encode_picks_reserve        the scratch of such calls with at most max_items entries of at most max_len bytes and at
 *                                   most max_bytes bytes between them
 *   rcx_encode_picks_scratch_bytes  what rcx_ctx_scratch_bytes reports for a fresh context after that reservation
 *   rcx_encode_picks                the same on host buffers: copy in, run, synchronise, copy out
 *
 * The tables.  d_src_at and d_src_len have max_items entries of uint64_t, d_count is one uint64_t.  Only entries
 * k < min(*d_count, max_items) are read; the others may hold anything.  A *d_count above max_items is treated as max_items
 * and latches RCX_E_CAPACITY at position max_items.  Sources may overlap or repeat and may have any alignment.
 *
 * The output.  d_comp_offsets[0 .. max_items] is written whole, in the caller's order: an entry of length 0, a skipped entry
 * and every entry at or behind the count has an empty stream, so the result is a valid stream set with nstreams = max_items
 * that rcx_decode_picks_device takes as it is.  Every stream is byte for byte what rcx_encode_items_device emits for the same
 * bytes.  Exactly [d_dst, d_dst + d_comp_offsets[max_items]) and the offsets table are written.
 *
 * Validation is the device's, because the tables are.  In this order, for entry k of length len > 0:
 *     len > max_len                                                             skipped, RCX_E_CORRUPT at k
 *     d_src_at[k] > src_cap or len > src_cap - d_src_at[k]                      skipped, RCX_E_CAPACITY at k
 * Every other entry is unaffected.  If the lengths of the valid entries sum to more than the promised max_bytes, nothing is
 * encoded: every offset is 0 and RCX_E_CAPACITY is latched at the count.  If the compacted streams take more than dst_cap
 * bytes, RCX_E_CAPACITY is latched at the count, the offsets are still written whole and nothing outside [d_dst, d_dst +
 * dst_cap) is (streams that would cross the end are left out), as with rcx_encode_items_device.  Failures are latched like
 * every other: rcx_ctx_sync_status returns RCX_E_CORRUPT if anything was corrupt, else RCX_E_CAPACITY, and the lowest failing
 * position of any kind.
 *
 * RCX_E_ARG, before anything is enqueued, is what the host can see: a null pointer, a bad coder, max_len > RCX_MAX_BLOCK,
 * max_items > 2^31 - 1.  max_items = 0 is RCX_OK and enqueues nothing.
 *
 * Scratch and graphs.  A scratch slot must hold the worst case of its entry's length, and a wave addresses its slots with one
 * stride: the planner lays the work order out in units of 64 entries, every power-of-two length class (16, 32, ... 2^24)
 * begins a unit, and a unit carries the stride of its class -- at most twice what the entry needs, and never
 * max_items * bound(max_len).  rcx_encode_picks_reserve makes the scratch, gives the kernels that want it their leave for
 * dynamic LDS and builds the divisor table for max_len symbols (the two range coders); after it a call with the same or smaller
 * max_items, max_len and max_bytes allocates nothing: it is a fixed sequence of kernel launches on `stream` and nothing else
 * (no memset, no copy), whose number and shapes depend on max_items alone, and may be captured.  Without a sufficient reservation
 * the call grows the scratch itself, which under capture is the caller's error, as with rcx_ctx_reserve.  The table scratch is
 * the one the other item calls use: calls of a context follow one another on one stream.
 *
 * With P = max_items + 1408 work positions (21 classes, each padded to a unit, and the launch rounded up to one):
 *     tables   = 20 * P + 16 + 8 * max_items + (2 * 4352 + 4) * 4
 *     slots    = 3 * max_bytes + 2112 * max_items + 256            (adaptive, static)
 *                4 * max_bytes + 1152 * max_items + 256            (the rANS coders)
 *     entries  = 2 * 4 * (P + 1)     sizes, redo                   (+ 4 * (P + 1) starts: the rANS coders;
 *                                                                    + 3104 * P models: RCX_CODER_RANS)
 *     rcx_encode_picks_scratch_bytes = tables + slots + entries    (0 for bad arguments or max_items = 0)
 * It is linear in max_items and in max_bytes and does not depend on max_len (the divisor tables are not part of
 * rcx_ctx_scratch_bytes).  The slot term follows from rcx_block_bound_for: a class's upper length U is at most
 * max(16, 2 * len - 1) <= 2 * len + 14, the range coders' bound is at most U * (1 + 1/32 + 1/8) + 2063 <= 3 * len + 2112, the
 * rANS coders' 2 * U + 1111 <= 4 * len + 1152.
 *
 * Work order.  As rcx_picks.h: long chains first, entries of similar length on one wave, by counting; the order of entries
 * within a bin differs from call to call and no output depends on it.
 *
 * The host-buffer call takes every one of the nitems entries as meant (max_items = nitems, max_bytes = the sum of the valid
 * lengths), writes comp_offsets[0 .. nitems] and *dst_size = comp_offsets[nitems], copies min(*dst_size, dst_cap) bytes to
 * dst and returns the latched status; the good entries are written also then.
 */
#ifndef RCX_ENCODE_PICKS_H_
#define RCX_ENCODE_PICKS_H_

#include "rcx.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_encode_picks_reserve(rcx_ctx* ctx, int coder, uint64_t max_items, uint32_t max_len, uint64_t max_bytes);
uint64_t rcx_encode_picks_scratch_bytes(int coder, uint64_t max_items, uint32_t max_len, uint64_t max_bytes);
int rcx_encode_picks_device(rcx_ctx* ctx, int coder, const void* d_src, uint64_t src_cap, const uint64_t* d_src_at, const uint64_t* d_src_len,
                            const uint64_t* d_count, uint64_t max_items, uint32_t max_len, uint64_t max_bytes, void* d_dst, uint64_t dst_cap,
                            uint64_t* d_comp_offsets, void* stream);
int rcx_encode_picks(rcx_ctx* ctx, int coder, const uint8_t* src, uint64_t src_cap, const uint64_t* src_at, const uint64_t* src_len, uint64_t nitems,
                     uint32_t max_len, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* comp_offsets);

#ifdef __cplusplus
}
#endif

#endif /* RCX_ENCODE_PICKS_H_ */
