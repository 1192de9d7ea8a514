"""ctypes binding of include/rcx_typed_stats.h: the order-0 cost of every candidate transform of every item, in one pass.

An item is that of base_items.py -- len bytes with an element width (1, 2, 4 or 8) and, for the op candidates, a base span of
len bytes at base_offsets[i] of a second buffer.  A candidate is the predictor's number or 3 + the base op's number: NONE,
DELTA, ZIGZAG, XOR, SUB, SUBZZ = 0 .. 5.  masks[i]: bit c asks for candidate c of item i.  cost[i, c] = the sum of
stats.cost_numpy over the sub-items (typed_items.sub_offsets) of item i as base_items.split would write it with that predictor
or op, 0 for a candidate that was not asked for.  include/rcx_typed_stats.h has the contract in full.

costs_numpy is that composition in numpy -- the mirror the tests hold the kernel to, and what somebody without a GPU decides
with (container.choose_delta_items_from_costs).  The calls themselves are host plumbing like rcx.py: the signatures are set on
rcx.lib()'s handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import base_items, rcx, stats, typed_items

NONE, DELTA, ZIGZAG, XOR, SUB, SUBZZ = range(6)  # include/rcx_typed_stats.h: RCX_CAND_*
CANDS = 6
NAMES = (None, "delta", "zigzag", "xor", "sub", "subzz")  # the names container.py and layout.py use, by candidate
PRED_BITS = 0x06
OP_BITS = 0x38
ALL_PREDS = 0x07  # none and the two predictors
ALL_OPS = 0x39    # none and the three ops
ALL = 0x3F

# every symbol include/rcx_typed_stats.h declares
EXPORTS = ("rcx_typed_stats_check", "rcx_typed_stats_items_device", "rcx_typed_stats_items")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the three calls of include/rcx_typed_stats.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_typed_stats_check.restype, L.rcx_typed_stats_check.argtypes = i32, [vp, vp, vp, vp, u64]
        # ctx, src, base, offsets, base offsets, widths, masks, n, cost, stream
        L.rcx_typed_stats_items_device.restype, L.rcx_typed_stats_items_device.argtypes = i32, [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp]
        # ctx, src, base, base bytes, offsets, base offsets, widths, masks, n, cost
        L.rcx_typed_stats_items.restype, L.rcx_typed_stats_items.argtypes = i32, [vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]
        _ready = True
    return L


def _tables(src_offsets, base_offsets, widths, masks):
    """-> (offsets uint64[nitems + 1], base offsets uint64[nitems] or None, widths, masks uint8[nitems] or None), contiguous."""
    offs, w, _ = typed_items._tables(src_offsets, widths, None)
    m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8)
    b = None if base_offsets is None else np.ascontiguousarray(base_offsets, dtype=np.uint64)
    if (m is not None and len(m) != len(w)) or (b is not None and len(b) != len(w)):
        raise ValueError("one mask and one base offset per item")
    return offs, b, w, m


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- the table, in numpy -----------------------------------------------------------------------------------------------------
def _sub_costs(y: np.ndarray, sub_offs: np.ndarray) -> np.ndarray:
    """The order-0 cost of every sub-item [sub_offs[k], sub_offs[k + 1]) of y -> uint64[nsub] (np.bincount over a few thousand
    sub-items at a time, stats.cost_numpy on the rows)."""
    nsub = len(sub_offs) - 1
    out = np.zeros(nsub, np.uint64)
    lens = np.diff(sub_offs)
    step = 4096
    for k0 in range(0, nsub, step):
        k1 = min(nsub, k0 + step)
        a, b = int(sub_offs[k0]), int(sub_offs[k1])
        if b == a:
            continue
        row = np.repeat(np.arange(k1 - k0, dtype=np.int64), lens[k0:k1])
        hist = np.bincount(row * 256 + y[a:b].astype(np.int64), minlength=(k1 - k0) * 256).reshape(k1 - k0, 256)
        out[k0:k1] = stats.cost_numpy(hist)
    return out


def costs_numpy(x, ref, src_offsets, base_offsets, widths, masks) -> np.ndarray:
    """x: bytes; item i = x[src_offsets[i] : src_offsets[i + 1]], its base span ref[base_offsets[i] :][: len] -> uint64
    [nitems, 6]: per candidate base_items.split_numpy of the items that ask for it, cut at typed_items.sub_offsets_numpy, the
    sub-items' stats.cost_numpy summed per item; 0 where the candidate was not asked for."""
    x = rcx._np_u8(x)
    offs, boffs, w, m = _tables(src_offsets, base_offsets, widths, masks)
    nitems = len(w)
    out = np.zeros((nitems, CANDS), np.uint64)
    if nitems == 0:
        return out
    if m is None or np.any(m >> CANDS) or np.any((w == 1) & ((m & PRED_BITS) != 0)):
        raise ValueError("a mask has bits 0 .. 5, and a width-1 item no predictor bit")
    sub_offs = typed_items.sub_offsets_numpy(offs, w).astype(np.int64)
    borders = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    for c in range(CANDS):
        asked = (m >> c & 1).astype(bool)
        if not asked.any():
            continue
        preds = np.where(asked, c, 0).astype(np.uint8) if c in (DELTA, ZIGZAG) else None
        ops = np.where(asked, c - XOR, base_items.NO_BASE).astype(np.uint8) if c >= XOR else None
        y = base_items.split_numpy(x, ref, offs, boffs, w, preds, ops)
        running = np.concatenate([[0], np.cumsum(_sub_costs(y, sub_offs), dtype=np.uint64)]).astype(np.uint64)
        out[:, c] = np.where(asked, running[borders[1:]] - running[borders[:-1]], 0)
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def check(src_offsets, base_offsets, widths, masks) -> int:
    """rcx_typed_stats_check: rcx.OK or rcx.E_ARG for the tables alone."""
    offs, b, w, m = _tables(src_offsets, base_offsets, widths, masks)
    return int(lib().rcx_typed_stats_check(offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(m), len(w)))


def items_device(ctx, src, ref, src_offsets, base_offsets, widths, masks, cost, stream=None) -> None:
    """src, ref: uint8 cuda tensors (ref may be None where no mask has an op bit); cost: an 8-byte cuda tensor [>= 6 * nitems],
    apart from both; the offsets, widths and masks: HOST tables.  cost[6 * i + c] = the cost of candidate c of item i, 0 if
    masks[i] lacks bit c.  Enqueues only; cannot be captured."""
    offs, b, w, m = _tables(src_offsets, base_offsets, widths, masks)
    if len(offs) and int(offs[-1]) > src.numel():
        raise ValueError("the offsets run past src")
    if cost.element_size() != 8 or cost.numel() < CANDS * len(w):
        raise ValueError("cost needs six 8-byte entries an item")
    if ref is not None and m is not None and b is not None:
        lens = np.diff(offs.astype(np.int64))
        used = ((m & OP_BITS) != 0) & (lens > 0)
        if used.any() and int((b.astype(np.int64)[used] + lens[used]).max()) > ref.numel():
            raise ValueError("a base span runs past the base")
    st = lib().rcx_typed_stats_items_device(ctx._h, src.data_ptr(), None if ref is None else ref.data_ptr(), offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(m),
                                            len(w), cost.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, "rcx_typed_stats_items_device")


def items(ctx, data, ref, src_offsets, base_offsets, widths, masks) -> np.ndarray:
    """Host bytes and their base -> cost uint64 [nitems, 6] (copy in, the kernels, copy out)."""
    src = rcx._np_u8(data)
    ref = None if ref is None else np.ascontiguousarray(rcx._np_u8(ref))
    offs, b, w, m = _tables(src_offsets, base_offsets, widths, masks)
    if len(offs) and int(offs[-1]) > len(src):
        raise ValueError("the offsets run past the buffer")
    cost = np.zeros((len(w), CANDS), np.uint64)
    st = lib().rcx_typed_stats_items(ctx._h, src.ctypes.data if len(src) else None, None if ref is None or not len(ref) else ref.ctypes.data,
                                     0 if ref is None else len(ref), offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(m), len(w), cost.ctypes.data)
    rcx._check(st, "rcx_typed_stats_items")
    return cost
