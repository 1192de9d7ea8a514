"""ctypes binding of include/rcx_planes.h: the byte-plane filter for typed data in front of the coders.

width = bytes per element (2, 4 or 8), block = the block size the coder will use afterwards.  A superblock is
width * block source bytes; within it plane p (byte p of every element) becomes one run of bytes, so that in a whole
superblock coder block s * width + p is exactly plane p.  include/rcx_planes.h has the transform in full.

The signatures are set on rcx.lib()'s handle; like rcx.py this is host plumbing, and there is no CPU fallback.  lib(),
_device and _host also serve predict.py, whose calls have one more argument in the middle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx

WIDTHS = (2, 4, 8)

# every symbol include/rcx_planes.h declares
EXPORTS = ("rcx_planes_split_device", "rcx_planes_join_device", "rcx_planes_split", "rcx_planes_join")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the eight calls of include/rcx_planes.h and include/rcx_predict.h set.  All eight
    are looked up at once, so a library from before the predictor (RCX_LIBRARY) fails here with an AttributeError, for the
    plane calls too."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        for stem, middle in (("rcx_planes_", [u32, u32]), ("rcx_predict_", [u32, u32, u32])):  # width, block(, pred)
            for call, last in (("split_device", [vp, vp]), ("join_device", [vp, vp]), ("split", [vp]), ("join", [vp])):
                getattr(L, stem + call).restype, getattr(L, stem + call).argtypes = i32, [vp, vp, u64, *middle, *last]
        _ready = True
    return L


def _device(name: str, ctx, src, dst, stream, *middle: int) -> None:
    if dst.numel() < src.numel():
        raise ValueError("dst needs as many bytes as src")
    st = getattr(lib(), name)(ctx._h, src.data_ptr(), src.numel(), *middle, dst.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, name)


def _host(name: str, ctx, data, *middle: int) -> bytes:
    src = rcx._np_u8(data)
    dst = np.empty(max(len(src), 1), dtype=np.uint8)
    rcx._check(getattr(lib(), name)(ctx._h, src.ctypes.data, len(src), *middle, dst.ctypes.data), name)
    return dst[: len(src)].tobytes()


def split_device(ctx, src, width: int, block: int, dst, stream=None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; dst[: src.numel()] = the planes of src.  Enqueues only."""
    _device("rcx_planes_split_device", ctx, src, dst, stream, width, block)


def join_device(ctx, src, width: int, block: int, dst, stream=None) -> None:
    """The inverse: src holds planes, dst[: src.numel()] = the elements.  Enqueues only."""
    _device("rcx_planes_join_device", ctx, src, dst, stream, width, block)


def split(ctx, data, width: int, block: int) -> bytes:
    """Host bytes -> their planes (copy in, one kernel, copy out)."""
    return _host("rcx_planes_split", ctx, data, width, block)


def join(ctx, data, width: int, block: int) -> bytes:
    return _host("rcx_planes_join", ctx, data, width, block)
