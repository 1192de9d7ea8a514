/*
 * rcx_stored_items.h -- stored items: the mix of rcx_stored.h behind the ITEM encode call, so that a set of item streams
 * never exceeds the items it holds (new; the reference has no batch format and no raw escape, so the C++ facades get nothing).
 *
 * Every coder writes a stream for every item that has bytes, whatever it codes to, and a stream carries 9 bytes of framing:
 * records and pages of a few dozen bytes all grow, and so do the low mantissa planes of floating-point tensors.  These calls
 * sit behind rcx_encode_items_device / rcx_encode_items (rcx.h, "Item calls"); the coders and their streams are untouched,
 * and the decode side is rcx_stored_decode_device (rcx_stored.h), which is in item geometry already.
 *
 * The rule is that of rcx_stored.h with the item in the block's place.  Item i is [src_offsets[i], src_offsets[i + 1]) of the
 * source, len_i bytes; its stream has coded_i = comp_offsets[i + 1] - comp_offsets[i] bytes; gain is 0 .. 65535:
 *
 *     stored_i  =  len_i > 0  &&  coded_i + floor(len_i * gain / 65536)  >=  len_i            in uint64_t
 *
 * A stored item's stream in the mixed set is its len_i raw bytes; a kept item's stream is unchanged.  A tie is stored.  AN
 * ITEM OF LENGTH 0 HAS NO STREAM AND IS NEVER STORED: its flag is 0, its mixed stream is empty, and its entry of the input
 * table is not looked at.  Every mixed stream is at most len_i bytes, so the mixed set is at most
 * src_offsets[nitems] - src_offsets[0] bytes: a dst_cap of that much is always enough.
 *
 * A worked example: four items, src_offsets = {0, 16, 16, 24, 64}, so len = 16, 0, 8, 40; the coder wrote streams of 20, 0, 8
 * and 21 bytes, comp_offsets = {0, 20, 20, 28, 49}.  With gain = 0: 20 >= 16 stored, the empty item never, 8 >= 8 stored (the
 * tie), 21 < 40 kept.
 *     d_stored  = {1, 0, 1, 0}
 *     d_offsets = {0, 16, 16, 24, 45}
 *     d_dst     = src[0 .. 16) | src[16 .. 24) | comp[28 .. 49)                  45 bytes where the coder wrote 49
 * With gain = 32768 (one half) item 3 is stored as well: 21 + 20 >= 40, d_offsets = {0, 16, 16, 24, 64}, d_dst = src; item 1
 * stays what it is under every gain.
 *
 *   rcx_stored_mix_items_device   behind rcx_encode_items_device on the same d_src and src_offsets: the coder's streams
 *                                 [d_comp, d_comp + comp_size) and table d_comp_offsets[0 .. nitems] -> the mixed streams,
 *                                 their table and one flag byte (0 or 1) an item, all in the caller's order
 *   rcx_stored_mix_items          the same on host buffers: copy in, run, synchronise, copy out
 *
 * mix.  src_offsets is a HOST table, as in the item calls: the work order is planned from it on the host (longest item
 * first; the items above 1024 bytes are copied by a workgroup each, the others by a wave each) and the tables go to the
 * device inside the call, SO IT CANNOT BE CAPTURED IN A GRAPH.  It only enqueues, on any stream; it uses the context's item
 * tables and size table, like the item encode call in front of it, so the two run on one stream or are ordered by the
 * caller.  It reads the items, the streams and their table and writes exactly [d_dst, d_dst + d_offsets[nitems]),
 * d_offsets[0 .. nitems] and d_stored[0 .. nitems); the byte buffers may have any alignment, the two device tables are
 * aligned for uint64_t.  nitems = 0, or all items empty, writes the zero table (and zero flags) and is RCX_OK.
 * RCX_E_ARG, before anything is enqueued: a src_offsets that is not monotonic; an item above RCX_MAX_BLOCK; gain > 65535;
 * nitems > 0x7FFFFFFF; a null pointer where bytes are needed (d_offsets always; src_offsets and d_stored with nitems > 0;
 * d_src, d_comp, d_comp_offsets and d_dst once an item has bytes); [d_dst, d_dst + dst_cap) overlapping the source span
 * [d_src + src_offsets[0], d_src + src_offsets[nitems]) or [d_comp, d_comp + comp_size).
 * Failures are latched like every other (rcx_ctx_sync_status): a dst_cap below the mixed size is RCX_E_CAPACITY, and no
 * stream that would end past dst_cap is written; an entry of d_comp_offsets that decreases or points past comp_size is not
 * followed -- RCX_E_CORRUPT at that item, whose mixed stream is empty and whose flag is 0, every other item unaffected.
 *
 * The host-buffer call follows rcx_stored_mix: it returns the mixed size in *dst_size (also when it is above dst_cap: then
 * RCX_E_CAPACITY and nothing copied out); `offsets` (nitems + 1) and `stored` (nitems) may be NULL.
 *
 * decode.  rcx_stored_decode_device(ctx, coder, d_dst, d_offsets[nitems], d_offsets, nitems, stored, pick, npick, dst_offsets,
 * d_out, stream) with the flags downloaded: a picked stored stream is copied, every other one decoded, picks in any order.
 */
#ifndef RCX_STORED_ITEMS_H_
#define RCX_STORED_ITEMS_H_

#include "rcx_stored.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_stored_mix_items_device(rcx_ctx* ctx, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, const void* d_comp,
                                uint64_t comp_size, const uint64_t* d_comp_offsets, uint32_t gain, void* d_dst, uint64_t dst_cap,
                                uint64_t* d_offsets, uint8_t* d_stored, void* stream);
int rcx_stored_mix_items(rcx_ctx* ctx, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems, const uint8_t* comp, uint64_t comp_size,
                         const uint64_t* comp_offsets, uint32_t gain, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* offsets,
                         uint8_t* stored);

#ifdef __cplusplus
}
#endif

#endif /* RCX_STORED_ITEMS_H_ */
