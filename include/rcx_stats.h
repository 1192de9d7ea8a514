/*
 * rcx_stats.h -- order-0 statistics of blocks or items on the GPU: every entry's 256 byte counts and its order-0 cost
 * (new; the reference has no such call, so the C++ facades get nothing).
 *
 * All four coders are order-0 with one model per block, so a block's byte histogram predicts what the block will code
 * to, to within a few percent, for the price of reading it once.  That is what decides between alternatives before
 * anything is coded: which predictor of rcx_predict.h pays off for a typed buffer (cpprcoder_amd/container.py,
 * pack_typed(..., predict="auto")), and later whether a block is worth coding at all.
 *
 * Geometry.  That of the rcx_crc32_* calls of rcx.h: the block calls cut [src, src + n) into blocks of `block` bytes,
 * RCX_MIN_BLOCK <= block <= RCX_MAX_BLOCK, the last one shorter, nblocks = rcx_block_count(n, block); the item calls
 * take item i = src[src_offsets[i] .. src_offsets[i + 1]), with src_offsets a HOST table of nitems + 1 ascending
 * entries also for the device call, and an item at most RCX_MAX_BLOCK bytes long.
 *
 *     hist[b * 256 + c]  the number of bytes equal to c in block or item b
 *     cost[b]            with m the entry's length and f_c its counts,
 *                            cost[b] = m * L(m) - sum over f_c > 0 of f_c * L(f_c)      in uint64_t:
 *                        the order-0 cost of the entry in bits, times 65536.  (cost + 65535) >> 16 bits, >> 19 bytes.
 *     L(x)               for 1 <= x <= 2^24: floor(log2(x) * 65536) by the square-and-compare recurrence
 *
 *         uint32_t L(uint32_t x)
 *         {
 *             uint32_t e = 31 - clz(x);                  // clz: the zero bits above the highest set bit of 32
 *             uint64_t m = (uint64_t)x << (31 - e);      // 2^31 <= m < 2^32
 *             uint32_t r = e;
 *             for (int i = 0; i < 16; ++i) {
 *                 m = (m * m) >> 31;
 *                 uint32_t bit = (uint32_t)(m >> 32);
 *                 m >>= bit;
 *                 r = 2 * r + bit;
 *             }
 *             return r;
 *         }
 *
 * This recurrence is the definition: every implementation gives these integers, and the tables of two machines are
 * equal.  L is monotone, so a cost is never negative.  L is never above the true logarithm and at most 1.00002 units of
 * 2^-16 below it (checked on 1 .. 2^17, 200 000 random values below 2^24 and the top 70 000).
 *     L(1) = 0   L(2) = 65536   L(3) = 103872   L(256) = 524288   L(65536) = 1048576   L(2^24 - 256) = 1572862
 * An empty item has cost 0 and a row of zeros.  A block of one repeated byte has cost 0; a block in which every byte value
 * occurs equally often has cost m * 8 * 65536.
 *
 *   rcx_stats_blocks_device   the tables of the blocks of d_src
 *   rcx_stats_items_device    the tables of the items of d_src
 * Either output may be NULL and is then not computed for the caller; both NULL is an error.  d_hist holds nblocks * 256
 * (nitems * 256) uint32_t, d_cost nblocks (nitems) uint64_t, each aligned for its type.
 *
 * The contract is that of the rcx_planes_* calls: the device calls only enqueue, on any stream and also under graph
 * capture (the block call; the item call sends its host table inside the call, exactly as rcx_crc32_items_device does);
 * they need no rcx_ctx_reserve and latch nothing.  They read exactly [d_src, d_src + n) -- the items' bytes -- at any
 * alignment and write exactly the two tables.  RCX_E_ARG, before anything is enqueued: a block outside the coders'
 * range, an item longer than RCX_MAX_BLOCK or a table that is not ascending, a null source with bytes to read, both
 * outputs null, an output that overlaps the source.  n = 0 (nitems = 0) is RCX_OK and does nothing.
 * The host-buffer variants copy in, run the kernel, synchronise and copy out.
 */
#ifndef RCX_STATS_H_
#define RCX_STATS_H_

#include "rcx.h"

#ifdef __cplusplus
extern "C" {
#endif

int rcx_stats_blocks_device(rcx_ctx* ctx, const void* d_src, uint64_t n, uint32_t block, uint32_t* d_hist, uint64_t* d_cost, void* stream);
int rcx_stats_items_device(rcx_ctx* ctx, const void* d_src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* d_hist, uint64_t* d_cost,
                           void* stream);
int rcx_stats_blocks(rcx_ctx* ctx, const uint8_t* src, uint64_t n, uint32_t block, uint32_t* hist, uint64_t* cost);
int rcx_stats_items(rcx_ctx* ctx, const uint8_t* src, const uint64_t* src_offsets, uint64_t nitems, uint32_t* hist, uint64_t* cost);

#ifdef __cplusplus
}
#endif

#endif /* RCX_STATS_H_ */
