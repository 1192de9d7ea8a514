"""ctypes binding of include/rcx_base.h: residuals against a base buffer, in front of the byte-plane filter.

width (1, 2, 4 or 8) and block are those of planes.py; width 1 has no planes.  `base` is a second buffer of the same length
that the reader holds as well: the checkpoint before, the base model, the last snapshot.  op: XOR (every element becomes
element ^ base element), SUB (element - base element, modulo 2^(8 * width)) or SUBZZ (SUB, and every difference d becomes
(d << 1) ^ -(d >> (8 * width - 1)), so that small differences of both signs become small numbers).  The residuals then go
through the plane split; join is the exact inverse with the same base.  Against an unrelated base data gets worse, so nobody
chooses it for the caller.  include/rcx_base.h has the transform in full.

split_numpy and join_numpy are that transform in numpy -- the mirror the tests hold the kernel to, and what somebody without a
GPU computes residuals with.  The calls themselves are host plumbing like rcx.py: the signatures are set on rcx.lib()'s handle,
and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx

WIDTHS = (1, 2, 4, 8)
XOR, SUB, SUBZZ = 0, 1, 2  # include/rcx_base.h: RCX_BASE_*
OPS = (XOR, SUB, SUBZZ)

# every symbol include/rcx_base.h declares
EXPORTS = ("rcx_base_split_device", "rcx_base_join_device", "rcx_base_split", "rcx_base_join")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_base.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        for call, last in (("split_device", [vp, vp]), ("join_device", [vp, vp]), ("split", [vp]), ("join", [vp])):
            f = getattr(L, "rcx_base_" + call)
            f.restype, f.argtypes = i32, [vp, vp, vp, u64, u32, u32, u32, *last]  # ctx, src, base, n, width, block, op, dst(, stream)
        _ready = True
    return L


# ---- the transform, in numpy -------------------------------------------------------------------------------------------------
def _zigzag(d):
    one = d.dtype.type(1)
    return (d << one) ^ (d.dtype.type(0) - (d >> d.dtype.type(8 * d.dtype.itemsize - 1)))


def _unzigzag(z):
    one = z.dtype.type(1)
    return (z >> one) ^ (z.dtype.type(0) - (z & one))


def _pair(x, ref, width: int, op: int):
    x, ref = np.ascontiguousarray(rcx._np_u8(x)), np.ascontiguousarray(rcx._np_u8(ref))
    if len(x) != len(ref):
        raise ValueError("the base has as many bytes as the data")
    if width not in WIDTHS or op not in OPS:
        raise ValueError("width 1, 2, 4 or 8; op XOR, SUB or SUBZZ")
    return x, ref


def split_numpy(x, ref, width: int, block: int, op: int) -> np.ndarray:
    """What rcx_base_split makes of x against ref: superblock by superblock (width * block bytes) the residuals of the whole
    elements, plane after plane, then the source's tail bytes."""
    x, ref = _pair(x, ref, width, op)
    out, dtype = x.copy(), np.dtype(f"<u{width}")  # (the R % width tail bytes of every superblock keep the source's values)
    for at in range(0, len(x), width * block):
        m = min(width * block, len(x) - at) // width
        e, b = x[at: at + m * width].view(dtype), ref[at: at + m * width].view(dtype)  # unsigned: numpy wraps modulo 2^(8 * width)
        r = e ^ b if op == XOR else e - b if op == SUB else _zigzag(e - b)
        out[at: at + m * width] = r.astype(dtype).view(np.uint8).reshape(m, width).T.reshape(-1)
    return out


def join_numpy(y, ref, width: int, block: int, op: int) -> np.ndarray:
    """The inverse, with the same ref."""
    y, ref = _pair(y, ref, width, op)
    out, dtype = y.copy(), np.dtype(f"<u{width}")
    for at in range(0, len(y), width * block):
        m = min(width * block, len(y) - at) // width
        r = np.ascontiguousarray(y[at: at + m * width].reshape(width, m).T).reshape(-1).view(dtype)
        b = ref[at: at + m * width].view(dtype)
        e = r ^ b if op == XOR else r + b if op == SUB else _unzigzag(r) + b
        out[at: at + m * width] = e.astype(dtype).view(np.uint8)
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def _device(name: str, ctx, src, ref, width: int, block: int, op: int, dst, stream) -> None:
    if ref.numel() != src.numel():
        raise ValueError("the base has as many bytes as src")
    if dst.numel() < src.numel():
        raise ValueError("dst needs as many bytes as src")
    st = getattr(lib(), name)(ctx._h, src.data_ptr(), ref.data_ptr(), src.numel(), width, block, op, dst.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, name)


def _host(name: str, ctx, data, ref, width: int, block: int, op: int) -> bytes:
    src, ref = rcx._np_u8(data), rcx._np_u8(ref)
    if len(ref) != len(src):
        raise ValueError("the base has as many bytes as the data")
    dst = np.empty(max(len(src), 1), dtype=np.uint8)
    rcx._check(getattr(lib(), name)(ctx._h, src.ctypes.data, ref.ctypes.data, len(src), width, block, op, dst.ctypes.data), name)
    return dst[: len(src)].tobytes()


def split_device(ctx, src, ref, width: int, block: int, op: int, dst, stream=None) -> None:
    """src, ref, dst: uint8 cuda tensors, dst apart from both; dst[: src.numel()] = the planes of the residuals of src against
    ref.  Enqueues only."""
    _device("rcx_base_split_device", ctx, src, ref, width, block, op, dst, stream)


def join_device(ctx, src, ref, width: int, block: int, op: int, dst, stream=None) -> None:
    """The inverse: src holds the residuals' planes, dst[: src.numel()] = the elements.  Enqueues only."""
    _device("rcx_base_join_device", ctx, src, ref, width, block, op, dst, stream)


def split(ctx, data, ref, width: int, block: int, op: int) -> bytes:
    """Host bytes and their base -> the planes of the residuals (copy both in, one kernel, copy out)."""
    return _host("rcx_base_split", ctx, data, ref, width, block, op)


def join(ctx, data, ref, width: int, block: int, op: int) -> bytes:
    return _host("rcx_base_join", ctx, data, ref, width, block, op)
