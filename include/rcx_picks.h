/*
 * rcx_picks.h -- item decode with every table in device memory: which streams, where their bytes go, how many entries are
 * meant and which streams are stored are read by the GPU, the call only enqueues, and it may be captured in a graph
 * (new; the reference decodes one buffer per call on the CPU, so the C++ facades get nothing).
 *
 * rcx_decode_items_device (rcx.h) and rcx_stored_decode_device (rcx_stored.h) take `pick`, `dst_offsets` and `stored` from
 * the HOST, plan on the CPU and upload the plan inside the call.  Here the plan is made by kernels (csrc/rcx_picks.hpp), so
 * a captured graph can be replayed against tables that another kernel rewrites between the replays, and the flags that
 * rcx_stored_mix_device or rcx_stored_mix_items_device left in device memory are used where they are.
 *
 *   rcx_decode_picks_device   entry k < *d_count decodes stream d_pick[k] of the set [d_comp, d_comp + comp_size) /
 *                             d_comp_offsets[0 .. nstreams] to d_dst[d_dst_at[k] .. d_dst_at[k] + d_dst_len[k])
 *   rcx_picks_reserve         the scratch of such calls with at most max_pick entries of at most max_len bytes
 *   rcx_picks_scratch_bytes   what rcx_ctx_scratch_bytes reports for a fresh context after that reservation
 *   rcx_decode_picks          the same on host buffers: copy in, run, synchronise, copy out
 *
 * The tables.  d_pick, d_dst_at and d_dst_len have max_pick entries of uint64_t, d_count is one uint64_t, d_stored is
 * nstreams bytes as the mix calls write them (non-zero: the stream is the item's raw bytes) or NULL for "none is stored".
 * Only entries k < min(*d_count, max_pick) are read; the others may hold anything.  A *d_count above max_pick is treated
 * as max_pick and latches RCX_E_CAPACITY at position max_pick.
 *
 * The rules of the item decode call hold: picks may repeat and need no order, an entry of length 0 is not looked at (not
 * even its pick), outputs may have any alignment, all four coders are covered, and a damaged stream is answered with the
 * status rcx_decode_items_device gives, the pick position k as its index.  Destinations are a position and a length, not a
 * prefix table, so that every entry can go to the slot an allocator chose; where the outputs of two entries overlap, the
 * bytes of the overlap are unspecified.  Nothing outside [d_dst, d_dst + dst_cap) is written, and nothing of d_dst that no
 * valid entry covers.
 *
 * Validation is the device's, because the tables are: a bad entry is not followed, as rcx_stored.h says of a bad entry of
 * d_comp_offsets.  In this order, for entry k of length len > 0:
 *     d_pick[k] >= nstreams, or len > max_len                                   skipped, RCX_E_CORRUPT at k
 *     d_dst_at[k] + len > dst_cap (in integers of any width)                    skipped, RCX_E_CAPACITY at k
 *     stream d_pick[k] is stored and is not exactly len bytes, or its
 *     offsets are out of order or leave the buffer                              skipped, RCX_E_CORRUPT at k
 * Nothing of a skipped entry is written and every other entry is unaffected.  Failures are latched like every other:
 * rcx_ctx_sync_status returns RCX_E_CORRUPT if anything was corrupt, else RCX_E_CAPACITY, and the lowest failing position
 * of any kind.
 *
 * RCX_E_ARG, before anything is enqueued, is what the host can see: a null pointer (d_stored apart), a bad coder, max_len >
 * RCX_MAX_BLOCK, max_pick or nstreams > 2^31 - 1.  max_pick = 0 is RCX_OK and enqueues nothing.
 *
 * Scratch and graphs.  The call needs the divisor table for max_len symbols (the two range coders), max_pick + 1 redo marks
 * and 24 bytes an entry + 34848 bytes of tables; rcx_picks_reserve makes them, and after it a call with the same or smaller
 * max_pick and max_len allocates nothing: it is a fixed sequence of kernel launches on `stream` and nothing else, whose shapes
 * depend on max_pick alone, and may be captured.  Without a sufficient reservation the call grows the scratch itself, which
 * under capture is the caller's error, as with rcx_ctx_reserve.  The table scratch is the one the host-planned item calls
 * upload into: calls of either kind on one context follow one another on one stream, as all calls of a context do.
 *     rcx_picks_scratch_bytes = max_pick * 24 + (2 * 4354 + 4) * 4 + (max_pick + 1) * 4        (0 for bad arguments or max_pick = 0)
 *
 * Work order.  The planner orders the entries as the host does -- long chains first, entries of similar length on one wave
 * -- by counting, not by sorting: lengths below 512 exactly, longer ones to 1 part in 256.  The order of entries within
 * such a class differs from call to call; no output depends on it.
 *
 * The host-buffer call reads and writes `dst` as a whole ([dst, dst + dst_cap) goes to the device and comes back), takes
 * every one of the npick entries as meant, and returns the latched status; the good entries are written also then.
 */
#ifndef RCX_PICKS_H_
#define RCX_PICKS_H_

#include "rcx.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_picks_reserve(rcx_ctx* ctx, int coder, uint64_t max_pick, uint32_t max_len);
uint64_t rcx_picks_scratch_bytes(int coder, uint64_t max_pick, uint32_t max_len);
int rcx_decode_picks_device(rcx_ctx* ctx, int coder, const void* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets, uint64_t nstreams,
                            const uint8_t* d_stored, const uint64_t* d_pick, const uint64_t* d_dst_at, const uint64_t* d_dst_len,
                            const uint64_t* d_count, uint64_t max_pick, uint32_t max_len, void* d_dst, uint64_t dst_cap, void* stream);
int rcx_decode_picks(rcx_ctx* ctx, int coder, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets, uint64_t nstreams,
                     const uint8_t* stored, const uint64_t* pick, const uint64_t* dst_at, const uint64_t* dst_len, uint64_t npick, uint32_t max_len,
                     uint8_t* dst, uint64_t dst_cap);

#ifdef __cplusplus
}
#endif

#endif /* RCX_PICKS_H_ */
