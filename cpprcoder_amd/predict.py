"""ctypes binding of include/rcx_predict.h: a delta predictor for typed integers in front of the byte-plane filter.

width and block are those of planes.py.  pred: NONE (the plane filter alone), DELTA (every element becomes its difference
to the element in front, modulo 2^(8 * width), restarting in every superblock of width * block bytes) or ZIGZAG (DELTA, and
every difference d becomes (d << 1) ^ -(d >> (8 * width - 1)), so that small negative differences become small numbers).
For integers whose differences are small -- sorted keys, CSR offsets, timestamps, sampled signals; unsorted data gets worse,
so nobody chooses it for the caller.  include/rcx_predict.h has the transform in full.

The signatures are set on rcx.lib()'s handle; like rcx.py this is host plumbing, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx

WIDTHS = (2, 4, 8)
NONE, DELTA, ZIGZAG = 0, 1, 2  # include/rcx_predict.h: RCX_PRED_*

# every symbol include/rcx_predict.h declares
EXPORTS = ("rcx_predict_split_device", "rcx_predict_join_device", "rcx_predict_split", "rcx_predict_join")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        for name in ("rcx_predict_split_device", "rcx_predict_join_device"):
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, u64, u32, u32, u32, vp, vp]
        for name in ("rcx_predict_split", "rcx_predict_join"):
            getattr(L, name).restype, getattr(L, name).argtypes = i32, [vp, vp, u64, u32, u32, u32, vp]
        _ready = True
    return L


def _device(name: str, ctx, src, width: int, block: int, pred: int, dst, stream) -> None:
    if dst.numel() < src.numel():
        raise ValueError("dst needs as many bytes as src")
    st = getattr(lib(), name)(ctx._h, src.data_ptr(), src.numel(), width, block, pred, dst.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, name)


def split_device(ctx, src, width: int, block: int, pred: int, dst, stream=None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; dst[: src.numel()] = the planes of the predicted src.  Enqueues only."""
    _device("rcx_predict_split_device", ctx, src, width, block, pred, dst, stream)


def join_device(ctx, src, width: int, block: int, pred: int, dst, stream=None) -> None:
    """The inverse: src holds predicted planes, dst[: src.numel()] = the elements.  Enqueues only."""
    _device("rcx_predict_join_device", ctx, src, width, block, pred, dst, stream)


def _host(name: str, ctx, data, width: int, block: int, pred: int) -> bytes:
    src = rcx._np_u8(data)
    dst = np.empty(max(len(src), 1), dtype=np.uint8)
    rcx._check(getattr(lib(), name)(ctx._h, src.ctypes.data, len(src), width, block, pred, dst.ctypes.data), name)
    return dst[: len(src)].tobytes()


def split(ctx, data, width: int, block: int, pred: int) -> bytes:
    """Host bytes -> the planes of their differences (copy in, one kernel, copy out)."""
    return _host("rcx_predict_split", ctx, data, width, block, pred)


def join(ctx, data, width: int, block: int, pred: int) -> bytes:
    return _host("rcx_predict_join", ctx, data, width, block, pred)
