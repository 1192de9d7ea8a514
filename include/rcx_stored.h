/*
 * rcx_stored.h -- stored blocks: a block whose stream did not shrink is kept as its raw bytes and decoded by copy
 * (new; the reference has no multi-block format and no raw escape, so the C++ facades get nothing).
 *
 * All four coders write a stream for every block, whatever it codes to: uniform bytes grow by a few hundred bytes a
 * block, and RCX_CODER_RANS8 doubles a block of one repeated byte.  These calls sit behind the block encode call and in
 * front of the decoders; the coders and their streams are untouched.
 *
 * The rule (integers only).  Block b of [src, src + n) cut into blocks of `block` bytes has len_b bytes; its stream has
 * coded_b = comp_offsets[b + 1] - comp_offsets[b] bytes; gain is 0 .. 65535, a fraction of the block in units of 1 / 65536:
 *
 *     stored_b  =  coded_b + floor(len_b * gain / 65536)  >=  len_b            in uint64_t
 *
 * A stored block's stream in the mixed set is its len_b raw bytes; a kept block's stream is unchanged.  gain = 0 stores
 * what does not shrink (a tie is stored: the copy decodes faster); a larger gain also stores what shrinks by less than that
 * fraction and so trades ratio for decode work -- 256 (0.39 %) stores a 65536-byte block that codes to 65280 or more.
 * Every mixed stream is at most len_b bytes, so the mixed set is at most n bytes: dst_cap >= n is always enough.
 *
 * A worked example: n = 40, block = 16, so len = 16, 16, 8; the coder wrote streams of 20, 9 and 8 bytes,
 * comp_offsets = {0, 20, 29, 37}.  With gain = 0: 20 >= 16 stored, 9 < 16 kept, 8 >= 8 stored (the tie).
 *     d_stored  = {1, 0, 1}
 *     d_offsets = {0, 16, 25, 33}
 *     d_dst     = src[0 .. 16) | comp[20 .. 29) | src[32 .. 40)                 33 bytes where the coder wrote 37
 * With gain = 32768 (one half) block 1 is stored as well: 9 + 8 >= 16, d_offsets = {0, 16, 32, 40}, d_dst = src.
 *
 *   rcx_stored_mix_device      behind rcx_encode_blocks_device on the same d_src, n and block: the coder's streams
 *                              [d_comp, d_comp + comp_size) and table d_comp_offsets[0 .. nblocks] -> the mixed streams,
 *                              their table and one flag byte (0 or 1) a block
 *   rcx_stored_decode_device   rcx_decode_items_device with one more HOST table: a picked stream st with stored[st] != 0
 *                              is copied to its output, every other picked stream is decoded
 *   rcx_stored_mix, rcx_stored_decode   the same on host buffers: copy in, run, synchronise, copy out
 *
 * mix.  Only enqueues, on any stream; it may be captured in a graph under the scratch rules of the block encode call (it
 * uses the context's size table, which that call on the same n and block has reserved).  It reads d_src, the streams and
 * their table and writes exactly [d_dst, d_dst + d_offsets[nblocks]), d_offsets[0 .. nblocks] and d_stored[0 .. nblocks);
 * the byte buffers may have any alignment, the two tables are aligned for uint64_t.  RCX_E_ARG, before anything is enqueued:
 * a block outside RCX_MIN_BLOCK .. RCX_MAX_BLOCK, gain > 65535, a null pointer with n > 0 (d_offsets always), [d_dst, d_dst +
 * dst_cap) overlapping [d_src, d_src + n) or [d_comp, d_comp + comp_size).  n = 0 writes d_offsets[0] = 0 and is RCX_OK.
 * Failures are latched like every other (rcx_ctx_sync_status): a dst_cap below the mixed size is RCX_E_CAPACITY, and no
 * stream that would end past dst_cap is written; an entry of d_comp_offsets that decreases or points past comp_size is not
 * followed -- RCX_E_CORRUPT at that block, whose mixed stream is empty.
 *
 * decode.  The shape and the rules of rcx_decode_items_device (rcx.h, "Item calls"): `pick` and `dst_offsets` are HOST
 * tables, picks may repeat and need not be ordered, a pick of length 0 is not looked at, the tables go to the device
 * inside the call, so it cannot be captured in a graph.  `stored` is a HOST table of nstreams bytes, or NULL for none: with
 * NULL or all zero the call is rcx_decode_items_device.  A stored stream whose length is not its output length, or whose
 * offsets are out of order or leave the buffer, is not copied: RCX_E_CORRUPT with the pick position, nothing of that entry
 * written, every other entry unaffected; rcx_ctx_sync_status reports the lowest failing position of either kind.  It reads
 * at most what the item call reads and writes exactly the picked output ranges.
 *
 * The host-buffer calls: rcx_stored_mix returns the mixed size in *dst_size (also when it is above dst_cap: then
 * RCX_E_CAPACITY and nothing copied out); `offsets` (nblocks + 1) and `stored` (nblocks) may be NULL.  rcx_stored_decode is
 * rcx_decode_items with the table.
 */
#ifndef RCX_STORED_H_
#define RCX_STORED_H_

#include "rcx.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_stored_mix_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t block, const void* d_comp, uint64_t comp_size,
                          const uint64_t* d_comp_offsets, uint32_t gain, void* d_dst, uint64_t dst_cap, uint64_t* d_offsets, uint8_t* d_stored,
                          void* stream);
int rcx_stored_decode_device(rcx_ctx* ctx, int coder, const void* d_comp, uint64_t comp_size, const uint64_t* d_comp_offsets, uint64_t nstreams,
                             const uint8_t* stored, const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, void* d_dst, void* stream);
int rcx_stored_mix(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t block, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets,
                   uint32_t gain, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_size, uint64_t* offsets, uint8_t* stored);
int rcx_stored_decode(rcx_ctx* ctx, int coder, const uint8_t* comp, uint64_t comp_size, const uint64_t* comp_offsets, uint64_t nstreams,
                      const uint8_t* stored, const uint64_t* pick, uint64_t npick, const uint64_t* dst_offsets, uint8_t* dst, uint64_t dst_cap);

#ifdef __cplusplus
}
#endif

#endif /* RCX_STORED_H_ */
