"""ctypes binding of include/rcx_base_items.h: residuals against a base per item, in front of the item calls.

An item is that of typed_items.py -- len bytes with an element width (1, 2, 4 or 8) -- and has either a predictor
(predict.NONE, DELTA, ZIGZAG), or a base op (base.XOR, SUB, SUBZZ) against len bytes at base_offsets[i] of a second buffer,
or neither (op NO_BASE).  With an op its transform is one superblock of include/rcx_base.h against its base span: the
residuals of the whole elements plane after plane, the len % width tail bytes as the source has them; without one it is
typed_items.py's.  The base spans are independent of the source's layout: any order, overlapping, one for many items.  The
coder's items behind it are typed_items.sub_offsets'.  include/rcx_base_items.h has the contract in full.

split_numpy and join_numpy are that transform in numpy, composed per item from base.split_numpy and typed_items.split_numpy
-- the mirror the tests hold the kernels to, and what somebody without a GPU transforms with.  The calls themselves are host
plumbing like rcx.py: the signatures are set on rcx.lib()'s handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import base, rcx, typed_items
from .base import SUB, SUBZZ, XOR  # noqa: F401  (part of this module's interface)
from .predict import DELTA, NONE, ZIGZAG  # noqa: F401

WIDTHS = (1, 2, 4, 8)
NO_BASE = 0xFF  # include/rcx_base_items.h: RCX_BASE_NONE
OPS = (XOR, SUB, SUBZZ, NO_BASE)

# every symbol include/rcx_base_items.h declares
EXPORTS = ("rcx_base_items_check", "rcx_base_items_hull", "rcx_base_items_split_device", "rcx_base_items_join_device", "rcx_base_items_split",
           "rcx_base_items_join")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the six calls of include/rcx_base_items.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_base_items_check.restype, L.rcx_base_items_check.argtypes = i32, [vp, vp, vp, vp, vp, u64]
        L.rcx_base_items_hull.restype, L.rcx_base_items_hull.argtypes = i32, [vp, vp, vp, vp, vp, u64, vp, vp]
        for name in ("rcx_base_items_split_device", "rcx_base_items_join_device"):  # ctx, src, base, offsets, base offsets, widths, preds, ops, n, dst, stream
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp]
        for name in ("rcx_base_items_split", "rcx_base_items_join"):  # ctx, src, base, base bytes, offsets, base offsets, widths, preds, ops, n, dst
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp]
        _ready = True
    return L


def _tables(src_offsets, base_offsets, widths, preds, ops):
    """-> (offsets uint64[nitems + 1], base offsets uint64[nitems] or None, widths, preds or None, ops or None), contiguous."""
    offs, w, p = typed_items._tables(src_offsets, widths, preds)
    o = None if ops is None else np.ascontiguousarray(ops, dtype=np.uint8)
    b = None if base_offsets is None else np.ascontiguousarray(base_offsets, dtype=np.uint64)
    if (o is not None and len(o) != len(w)) or (b is not None and len(b) != len(w)):
        raise ValueError("one op and one base offset per item")
    return offs, b, w, p, o


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- the transform, in numpy -------------------------------------------------------------------------------------------------
def _transform(x, ref, src_offsets, base_offsets, widths, preds, ops, forward: bool) -> np.ndarray:
    x = rcx._np_u8(x)
    offs, boffs, w, p, o = _tables(src_offsets, base_offsets, widths, preds, ops)
    # the items without an op: typed_items' transform, with the others as plain bytes (width 1 is a copy there)
    based = np.zeros(len(w), bool) if o is None else o != NO_BASE
    out = typed_items._transform(x, offs, np.where(based, 1, w), None if p is None else np.where(based, 0, p), forward)
    if not based.any():
        return out
    ref = rcx._np_u8(ref) if ref is not None else np.zeros(0, np.uint8)
    for i in np.flatnonzero(based):
        a, b, width, op = int(offs[i]), int(offs[i + 1]), int(w[i]), int(o[i])
        if width not in WIDTHS or op not in base.OPS or (p is not None and p[i]) or b < a:
            raise ValueError(f"item {i}: width {width}, op {op}, bytes {a}..{b}")
        if b == a:
            continue
        if boffs is None or int(boffs[i]) + (b - a) > len(ref):
            raise ValueError(f"item {i}: its base span runs past the base")
        span = ref[int(boffs[i]): int(boffs[i]) + (b - a)]
        # one superblock: a block of m + 1 elements holds the item's m elements and its tail
        out[a:b] = (base.split_numpy if forward else base.join_numpy)(x[a:b], span, width, (b - a) // width + 1, op)
    return out


def split_numpy(x, ref, src_offsets, base_offsets, widths, preds=None, ops=None) -> np.ndarray:
    """x: bytes; item i = x[src_offsets[i] : src_offsets[i + 1]], its base span ref[base_offsets[i] :][: len] where ops[i] is not
    NO_BASE -> the buffer with every item transformed (uint8, len(x))."""
    return _transform(x, ref, src_offsets, base_offsets, widths, preds, ops, True)


def join_numpy(y, ref, src_offsets, base_offsets, widths, preds=None, ops=None) -> np.ndarray:
    return _transform(y, ref, src_offsets, base_offsets, widths, preds, ops, False)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def check(src_offsets, base_offsets, widths, preds=None, ops=None) -> int:
    """rcx_base_items_check: rcx.OK or rcx.E_ARG for the tables alone."""
    offs, b, w, p, o = _tables(src_offsets, base_offsets, widths, preds, ops)
    return int(lib().rcx_base_items_check(offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(p), _ptr(o), len(w)))


def hull(src_offsets, base_offsets, widths, preds=None, ops=None) -> tuple:
    """rcx_base_items_hull: (lo, hi) of the base spans in use, (0, 0) where no item with an op has bytes."""
    offs, b, w, p, o = _tables(src_offsets, base_offsets, widths, preds, ops)
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    rcx._check(lib().rcx_base_items_hull(offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(p), _ptr(o), len(w), C.byref(lo), C.byref(hi)), "rcx_base_items_hull")
    return int(lo.value), int(hi.value)


def _device(name: str, ctx, src, ref, src_offsets, base_offsets, widths, preds, ops, dst, stream) -> None:
    offs, b, w, p, o = _tables(src_offsets, base_offsets, widths, preds, ops)
    if len(offs) and (int(offs[-1]) > src.numel() or int(offs[-1]) > dst.numel()):
        raise ValueError("the offsets run past src or dst")
    if ref is not None and o is not None and b is not None:
        lens = np.diff(offs.astype(np.int64))
        used = (o != NO_BASE) & (lens > 0)
        if used.any() and int((b.astype(np.int64)[used] + lens[used]).max()) > ref.numel():
            raise ValueError("a base span runs past the base")
    st = getattr(lib(), name)(ctx._h, src.data_ptr(), None if ref is None else ref.data_ptr(), offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(p), _ptr(o),
                              len(w), dst.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, name)


def split_device(ctx, src, ref, src_offsets, base_offsets, widths, preds, ops, dst, stream=None) -> None:
    """src, ref, dst: uint8 cuda tensors, dst apart from src and from the hull of the base spans in use (ref may be None where
    ops is); the offsets, widths, preds and ops (or None): HOST tables.  The bytes of every item of dst = the transform of that
    item of src.  Enqueues only; cannot be captured."""
    _device("rcx_base_items_split_device", ctx, src, ref, src_offsets, base_offsets, widths, preds, ops, dst, stream)


def join_device(ctx, src, ref, src_offsets, base_offsets, widths, preds, ops, dst, stream=None) -> None:
    """The inverse, with the same base.  Enqueues only; cannot be captured."""
    _device("rcx_base_items_join_device", ctx, src, ref, src_offsets, base_offsets, widths, preds, ops, dst, stream)


def _host(name: str, ctx, data, ref, src_offsets, base_offsets, widths, preds, ops) -> bytes:
    src = rcx._np_u8(data)
    ref = None if ref is None else np.ascontiguousarray(rcx._np_u8(ref))
    offs, b, w, p, o = _tables(src_offsets, base_offsets, widths, preds, ops)
    if len(offs) and int(offs[-1]) > len(src):
        raise ValueError("the offsets run past the buffer")
    dst = src.copy() if len(src) else np.zeros(1, np.uint8)  # (bytes no item covers stay)
    st = getattr(lib(), name)(ctx._h, src.ctypes.data, None if ref is None or not len(ref) else ref.ctypes.data, 0 if ref is None else len(ref),
                              offs.ctypes.data, _ptr(b), w.ctypes.data, _ptr(p), _ptr(o), len(w), dst.ctypes.data)
    rcx._check(st, name)
    return dst[: len(src)].tobytes()


def split(ctx, data, ref, src_offsets, base_offsets, widths, preds=None, ops=None) -> bytes:
    """Host bytes and their base -> every item transformed (copy in, the kernels, copy out)."""
    return _host("rcx_base_items_split", ctx, data, ref, src_offsets, base_offsets, widths, preds, ops)


def join(ctx, data, ref, src_offsets, base_offsets, widths, preds=None, ops=None) -> bytes:
    return _host("rcx_base_items_join", ctx, data, ref, src_offsets, base_offsets, widths, preds, ops)
