"""ctypes binding of include/rcx_typed_items.h: the byte-plane filter and the predictor per item, in front of the item calls.

A typed item is len bytes with an element width (1, 2, 4 or 8) and a predictor (predict.NONE, DELTA, ZIGZAG) of its own.
Its transform is that of one superblock of include/rcx_planes.h / rcx_predict.h with m = len // width elements: the
predictor starts at 0 in front of the item's first element, plane p goes to [p * m, (p + 1) * m) of the item's span, the
len % width tail bytes keep their places; width 1 is a copy.  The coder's items behind it are the sub-items: an item's width
planes in order, the last one with the tail (sub_offsets).  include/rcx_typed_items.h has the contract in full.

split_numpy and join_numpy are that arithmetic in numpy -- the mirror the tests hold the kernels to, and what somebody
without a GPU transforms with.  The calls themselves are host plumbing like rcx.py: the signatures are set on rcx.lib()'s
handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .predict import DELTA, NONE, ZIGZAG  # noqa: F401  (part of this module's interface)

WIDTHS = (1, 2, 4, 8)

# every symbol include/rcx_typed_items.h declares
EXPORTS = ("rcx_typed_items_sub_count", "rcx_typed_items_sub_offsets", "rcx_typed_items_split_device", "rcx_typed_items_join_device",
           "rcx_typed_items_split", "rcx_typed_items_join")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the six calls of include/rcx_typed_items.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_typed_items_sub_count.restype, L.rcx_typed_items_sub_count.argtypes = u64, [vp, u64]
        L.rcx_typed_items_sub_offsets.restype, L.rcx_typed_items_sub_offsets.argtypes = i32, [vp, vp, u64, vp]
        for name in ("rcx_typed_items_split_device", "rcx_typed_items_join_device"):
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, vp, vp, vp, u64, vp, vp]
        for name in ("rcx_typed_items_split", "rcx_typed_items_join"):
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, vp, vp, vp, u64, vp]
        _ready = True
    return L


def _tables(src_offsets, widths, preds):
    """-> (offsets uint64[nitems + 1], widths uint8[nitems], preds uint8[nitems] or None), contiguous."""
    offs = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    nitems = len(offs) - 1
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    p = None if preds is None else np.ascontiguousarray(preds, dtype=np.uint8)
    if nitems < 0 or len(w) != nitems or (p is not None and len(p) != nitems):
        raise ValueError("one width (and one predictor) per item, and nitems + 1 offsets")
    return offs, w, p


# ---- the arithmetic, in numpy ------------------------------------------------------------------------------------------------
def sub_offsets_numpy(src_offsets, widths) -> np.ndarray:
    """The table of the sub-items: item i gives widths[i] of them, len // width bytes each, the last with the len % width tail."""
    offs = np.asarray(src_offsets, dtype=np.uint64).astype(np.int64)
    w = np.asarray(widths, dtype=np.int64)
    if np.any(~np.isin(w, WIDTHS)):
        raise ValueError("a width is 1, 2, 4 or 8")
    lens = np.diff(offs)
    m = lens // np.maximum(w, 1)
    sub = np.repeat(m, w)
    last = np.cumsum(w) - 1
    if len(w):
        sub[last] += lens - m * w
    out = np.empty(len(sub) + 1, dtype=np.uint64)
    out[0] = offs[0] if len(offs) else 0
    out[1:] = (offs[0] if len(offs) else 0) + np.cumsum(sub)
    return out


def _zigzag(d):
    one = d.dtype.type(1)
    return (d << one) ^ (d.dtype.type(0) - (d >> d.dtype.type(8 * d.dtype.itemsize - 1)))


def _unzigzag(z):
    one = z.dtype.type(1)
    return (z >> one) ^ (z.dtype.type(0) - (z & one))


def _transform(x, src_offsets, widths, preds, forward: bool) -> np.ndarray:
    x = rcx._np_u8(x)
    offs, w, p = _tables(src_offsets, widths, preds)
    if len(offs) and int(offs[-1]) > len(x):
        raise ValueError("the offsets run past the buffer")
    out = x.copy()  # (what no item covers, and every tail, stays)
    for i in range(len(w)):
        a, b, width, pred = int(offs[i]), int(offs[i + 1]), int(w[i]), 0 if p is None else int(p[i])
        if width not in WIDTHS or pred > ZIGZAG or (width == 1 and pred) or b < a:
            raise ValueError(f"item {i}: width {width}, predictor {pred}, bytes {a}..{b}")
        m = (b - a) // width
        if m == 0 or width == 1:
            continue
        dtype = np.dtype(f"<u{width}")
        if forward:
            e = x[a: a + m * width].view(dtype)
            if pred:
                d = e.copy()
                d[1:] = e[1:] - e[:-1]  # d_0 = e_0: the predictor starts at 0 in front of the item
                e = _zigzag(d) if pred == ZIGZAG else d
            out[a: a + m * width] = e.view(np.uint8).reshape(m, width).T.reshape(-1)
        else:
            e = np.ascontiguousarray(x[a: a + m * width].reshape(width, m).T).reshape(-1).view(dtype)
            if pred:
                e = np.cumsum(_unzigzag(e) if pred == ZIGZAG else e, dtype=dtype)
            out[a: a + m * width] = e.astype(dtype).view(np.uint8)
    return out


def split_numpy(x, src_offsets, widths, preds=None) -> np.ndarray:
    """x: bytes; item i = x[src_offsets[i] : src_offsets[i + 1]] -> the buffer with every item transformed (uint8, len(x))."""
    return _transform(x, src_offsets, widths, preds, True)


def join_numpy(y, src_offsets, widths, preds=None) -> np.ndarray:
    return _transform(y, src_offsets, widths, preds, False)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def sub_count(widths) -> int:
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    return int(lib().rcx_typed_items_sub_count(w.ctypes.data, len(w)))


def sub_offsets(src_offsets, widths) -> np.ndarray:
    """rcx_typed_items_sub_offsets: the src_offsets the item calls take behind a split (uint64, sum of the widths + 1)."""
    offs, w, _ = _tables(src_offsets, widths, None)
    out = np.zeros(int(w.astype(np.int64).sum()) + 1, dtype=np.uint64)
    rcx._check(lib().rcx_typed_items_sub_offsets(offs.ctypes.data, w.ctypes.data, len(w), out.ctypes.data), "rcx_typed_items_sub_offsets")
    return out


def _device(name: str, ctx, src, src_offsets, widths, preds, dst, stream) -> None:
    offs, w, p = _tables(src_offsets, widths, preds)
    if len(offs) and (int(offs[-1]) > src.numel() or int(offs[-1]) > dst.numel()):
        raise ValueError("the offsets run past src or dst")
    st = getattr(lib(), name)(ctx._h, src.data_ptr(), offs.ctypes.data, w.ctypes.data, None if p is None else p.ctypes.data, len(w), dst.data_ptr(),
                              ctx._stream_handle(stream))
    rcx._check(st, name)


def split_device(ctx, src, src_offsets, widths, preds, dst, stream=None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; src_offsets, widths, preds (or None): HOST tables.  The bytes of every
    item of dst = the transform of that item of src.  Enqueues only; cannot be captured."""
    _device("rcx_typed_items_split_device", ctx, src, src_offsets, widths, preds, dst, stream)


def join_device(ctx, src, src_offsets, widths, preds, dst, stream=None) -> None:
    """The inverse.  Enqueues only; cannot be captured."""
    _device("rcx_typed_items_join_device", ctx, src, src_offsets, widths, preds, dst, stream)


def _host(name: str, ctx, data, src_offsets, widths, preds) -> bytes:
    src = rcx._np_u8(data)
    offs, w, p = _tables(src_offsets, widths, preds)
    if len(offs) and int(offs[-1]) > len(src):
        raise ValueError("the offsets run past the buffer")
    dst = src.copy() if len(src) else np.zeros(1, np.uint8)  # (bytes no item covers stay)
    st = getattr(lib(), name)(ctx._h, src.ctypes.data, offs.ctypes.data, w.ctypes.data, None if p is None else p.ctypes.data, len(w), dst.ctypes.data)
    rcx._check(st, name)
    return dst[: len(src)].tobytes()


def split(ctx, data, src_offsets, widths, preds=None) -> bytes:
    """Host bytes -> every item transformed (copy in, one kernel, copy out)."""
    return _host("rcx_typed_items_split", ctx, data, src_offsets, widths, preds)


def join(ctx, data, src_offsets, widths, preds=None) -> bytes:
    return _host("rcx_typed_items_join", ctx, data, src_offsets, widths, preds)
