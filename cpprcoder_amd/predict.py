"""ctypes binding of include/rcx_predict.h: a delta predictor for typed integers in front of the byte-plane filter.

width and block are those of planes.py.  pred: NONE (the plane filter alone), DELTA (every element becomes its difference
to the element in front, modulo 2^(8 * width), restarting in every superblock of width * block bytes) or ZIGZAG (DELTA, and
every difference d becomes (d << 1) ^ -(d >> (8 * width - 1)), so that small negative differences become small numbers).
For integers whose differences are small -- sorted keys, CSR offsets, timestamps, sampled signals; unsorted data gets worse,
so nobody chooses it for the caller.  include/rcx_predict.h has the transform in full.

planes.py has lib() and the two functions that make a call; like rcx.py this is host plumbing, and there is no CPU fallback.
"""
from __future__ import annotations

from .planes import WIDTHS, _device, _host, lib  # noqa: F401  (WIDTHS and lib are part of this module's interface)

NONE, DELTA, ZIGZAG = 0, 1, 2  # include/rcx_predict.h: RCX_PRED_*

# every symbol include/rcx_predict.h declares
EXPORTS = ("rcx_predict_split_device", "rcx_predict_join_device", "rcx_predict_split", "rcx_predict_join")


def split_device(ctx, src, width: int, block: int, pred: int, dst, stream=None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; dst[: src.numel()] = the planes of the predicted src.  Enqueues only."""
    _device("rcx_predict_split_device", ctx, src, dst, stream, width, block, pred)


def join_device(ctx, src, width: int, block: int, pred: int, dst, stream=None) -> None:
    """The inverse: src holds predicted planes, dst[: src.numel()] = the elements.  Enqueues only."""
    _device("rcx_predict_join_device", ctx, src, dst, stream, width, block, pred)


def split(ctx, data, width: int, block: int, pred: int) -> bytes:
    """Host bytes -> the planes of their differences (copy in, one kernel, copy out)."""
    return _host("rcx_predict_split", ctx, data, width, block, pred)


def join(ctx, data, width: int, block: int, pred: int) -> bytes:
    return _host("rcx_predict_join", ctx, data, width, block, pred)
