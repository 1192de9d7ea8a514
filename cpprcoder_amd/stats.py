"""ctypes binding of include/rcx_stats.h: the byte counts and the order-0 cost of every block or item, on the GPU.

hist[b * 256 + c] = how many bytes of block or item b equal c; cost[b] = m * L(m) - sum of f_c * L(f_c) over the counts
f_c > 0 of the entry's m bytes: its order-0 cost in bits, times 65536.  L(x) = floor(log2(x) * 65536) by sixteen
square-and-compare steps: integers throughout, the same on every machine.  include/rcx_stats.h has the contract in full.

log2_q16 and cost_numpy are that arithmetic in numpy uint64 -- the mirror the tests hold the kernel to, and what somebody
without a GPU computes costs with.  The calls themselves are host plumbing like rcx.py: the signatures are set on
rcx.lib()'s handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx

# every symbol include/rcx_stats.h declares
EXPORTS = ("rcx_stats_blocks_device", "rcx_stats_items_device", "rcx_stats_blocks", "rcx_stats_items")

UNIT = 1 << 16  # a cost counts bits in units of 1 / UNIT

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_stats.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.rcx_stats_blocks_device.restype, L.rcx_stats_blocks_device.argtypes = i32, [vp, vp, u64, u32, vp, vp, vp]
        L.rcx_stats_items_device.restype, L.rcx_stats_items_device.argtypes = i32, [vp, vp, vp, u64, vp, vp, vp]
        L.rcx_stats_blocks.restype, L.rcx_stats_blocks.argtypes = i32, [vp, vp, u64, u32, vp, vp]
        L.rcx_stats_items.restype, L.rcx_stats_items.argtypes = i32, [vp, vp, vp, u64, vp, vp]
        _ready = True
    return L


# ---- the arithmetic, in numpy ------------------------------------------------------------------------------------------------
def log2_q16(x) -> np.ndarray:
    """L(x) of include/rcx_stats.h for 1 <= x <= 2^24, elementwise -> uint64."""
    x = np.asarray(x, dtype=np.uint64)
    if x.size and (int(x.min()) < 1 or int(x.max()) > 1 << 24):
        raise ValueError("L(x) is defined for 1 <= x <= 2^24")
    e = np.zeros(x.shape, np.uint64)
    for s in (16, 8, 4, 2, 1):  # floor(log2 x): 31 - clz
        up = (x >> (e + np.uint64(s))) != 0
        e = e + np.where(up, np.uint64(s), np.uint64(0))
    m = x << (np.uint64(31) - e)
    r = e.copy()
    for _ in range(16):
        m = (m * m) >> np.uint64(31)  # below 2^64: m < 2^32
        bit = m >> np.uint64(32)
        m = m >> bit
        r = np.uint64(2) * r + bit
    return r


def cost_numpy(hist) -> np.ndarray:
    """hist: counts [..., 256] -> the cost of each row, uint64: m * L(m) - sum of f * L(f) over the counts above 0."""
    h = np.asarray(hist, dtype=np.uint64)
    if h.shape[-1] != 256:
        raise ValueError("a histogram has 256 counts")
    m = h.sum(axis=-1, dtype=np.uint64)

    def term(f):
        return f * log2_q16(np.maximum(f, np.uint64(1)))  # (L(1) = 0: a count of 0 adds nothing)

    return term(m) - term(h).sum(axis=-1, dtype=np.uint64)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def blocks_device(ctx, src, block: int, hist=None, cost=None, stream=None) -> None:
    """src: uint8 cuda tensor; hist: 4-byte cuda tensor [>= nblocks * 256] or None; cost: 8-byte cuda tensor [>= nblocks] or
    None (not both).  Enqueues only."""
    n = src.numel()
    if rcx.MIN_BLOCK <= block <= rcx.MAX_BLOCK:
        nblocks = rcx.block_count(n, block)
        if (hist is not None and hist.numel() < 256 * nblocks) or (cost is not None and cost.numel() < nblocks):
            raise ValueError("hist needs 256 entries a block and cost one")
    st = lib().rcx_stats_blocks_device(ctx._h, src.data_ptr(), n, block, _ptr(hist), _ptr(cost), ctx._stream_handle(stream))
    rcx._check(st, "rcx_stats_blocks_device")


def items_device(ctx, src, src_offsets, hist=None, cost=None, stream=None) -> None:
    """Item i = src[src_offsets[i] : src_offsets[i + 1]] (HOST table); hist [>= nitems * 256] and cost [>= nitems] as above.
    Enqueues only."""
    offs = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    nitems = len(offs) - 1
    if (hist is not None and hist.numel() < 256 * nitems) or (cost is not None and cost.numel() < nitems):
        raise ValueError("hist needs 256 entries an item and cost one")
    st = lib().rcx_stats_items_device(ctx._h, src.data_ptr(), offs.ctypes.data, nitems, _ptr(hist), _ptr(cost), ctx._stream_handle(stream))
    rcx._check(st, "rcx_stats_items_device")


def blocks(ctx, data, block: int):
    """Host bytes -> (hist uint32 [nblocks, 256], cost uint64 [nblocks]): copy in, one kernel, copy out."""
    src = rcx._np_u8(data)
    nblocks = rcx.block_count(len(src), block) if rcx.MIN_BLOCK <= block <= rcx.MAX_BLOCK else 0
    hist, cost = np.zeros((nblocks, 256), np.uint32), np.zeros(nblocks, np.uint64)
    rcx._check(lib().rcx_stats_blocks(ctx._h, src.ctypes.data, len(src), block, hist.ctypes.data, cost.ctypes.data), "rcx_stats_blocks")
    return hist, cost


def items(ctx, items, lengths=None):
    """items: a list of buffers, or one buffer with `lengths` cutting it -> (hist uint32 [nitems, 256], cost uint64 [nitems])."""
    if lengths is None:
        parts = [rcx._np_u8(x) for x in items]
        lengths = [len(x) for x in parts]
        src = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    else:
        src = rcx._np_u8(items)
    offs = rcx.item_offsets(lengths)
    if int(offs[-1]) != len(src):
        raise ValueError("lengths do not add up to the buffer")
    nitems = len(offs) - 1
    hist, cost = np.zeros((nitems, 256), np.uint32), np.zeros(nitems, np.uint64)
    rcx._check(lib().rcx_stats_items(ctx._h, src.ctypes.data, offs.ctypes.data, nitems, hist.ctypes.data, cost.ctypes.data), "rcx_stats_items")
    return hist, cost
