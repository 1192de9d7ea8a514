"""ctypes binding of include/rcx_stored.h: stored blocks -- a block whose stream did not shrink is kept as its raw bytes and
decoded by copy.

The rule, in integers: block b of len_b bytes whose stream has coded_b bytes is stored iff
    coded_b + floor(len_b * gain / 65536) >= len_b
with gain in 0 .. 65535.  gain = 0 stores what does not shrink (a tie is stored); a larger gain also stores what shrinks by
less than gain / 65536 of the block.  include/rcx_stored.h has the contract in full, and a worked example.

is_stored, mix_numpy and unmix_numpy are that rule and the two directions in numpy -- the mirror the tests hold the kernels
to, and what somebody without a GPU takes a container's payload apart with.  The calls themselves are host plumbing like
rcx.py: the signatures are set on rcx.lib()'s handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .layout import block_lengths  # noqa: F401 (len_b of every block: one rule for the containers and the mirror here)

# every symbol include/rcx_stored.h declares
EXPORTS = ("rcx_stored_mix_device", "rcx_stored_decode_device", "rcx_stored_mix", "rcx_stored_decode")

GAIN_ONE = 1 << 16  # a gain counts fractions of a block in units of 1 / GAIN_ONE
GAIN_MAX = GAIN_ONE - 1

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_stored.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.rcx_stored_mix_device.restype, L.rcx_stored_mix_device.argtypes = i32, [vp, vp, u64, u32, vp, u64, vp, u32, vp, u64, vp, vp, vp]
        L.rcx_stored_decode_device.restype, L.rcx_stored_decode_device.argtypes = i32, [vp, i32, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]
        L.rcx_stored_mix.restype, L.rcx_stored_mix.argtypes = i32, [vp, vp, u64, u32, vp, u64, vp, u32, vp, u64, vp, vp, vp]
        L.rcx_stored_decode.restype, L.rcx_stored_decode.argtypes = i32, [vp, i32, vp, u64, vp, u64, vp, vp, u64, vp, vp, u64]
        _ready = True
    return L


# ---- the rule and its two directions, in numpy -----------------------------------------------------------------------------------
def gain_q16(x) -> int:
    """What stored=x of container.pack means as a gain: True is 0 (store what does not shrink), a fraction 0 <= x < 1 of
    the block is min(65535, int(x * 65536))."""
    if x is True:
        return 0
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0 <= x < 1:
        raise ValueError("a gain is True or a fraction of the block, 0 <= g < 1")
    return min(GAIN_MAX, int(x * GAIN_ONE))


def is_stored(coded, length, gain: int):
    """The rule, elementwise (Python integers or arrays): coded + floor(length * gain / 65536) >= length."""
    if not 0 <= int(gain) <= GAIN_MAX:
        raise ValueError("a gain is 0 .. 65535")
    if isinstance(coded, (int, np.integer)) and isinstance(length, (int, np.integer)):
        return int(coded) + ((int(length) * int(gain)) >> 16) >= int(length)
    coded, length = np.asarray(coded, dtype=np.uint64), np.asarray(length, dtype=np.uint64)
    return coded + ((length * np.uint64(gain)) >> np.uint64(16)) >= length  # (below 2^64: length < 2^24, gain < 2^16)


def mix_numpy(src, block: int, payload, offsets, gain: int = 0):
    """What rcx_stored_mix writes -> (mixed payload uint8, its offsets uint64 [nblocks + 1], flags uint8 [nblocks])."""
    src, payload = rcx._np_u8(src), rcx._np_u8(payload)
    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = block_lengths(len(src), block)
    if len(offsets) != len(lengths) + 1:
        raise ValueError("one stream per block")
    flags = np.asarray(is_stored(np.diff(offsets), lengths, gain), dtype=bool).reshape(len(lengths))
    parts = [src[b * block: b * block + int(lengths[b])] if flags[b] else payload[int(offsets[b]): int(offsets[b + 1])] for b in range(len(lengths))]
    mixed = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=mixed[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), mixed, flags.astype(np.uint8)


def unmix_numpy(payload, offsets, stored, lengths, decode) -> np.ndarray:
    """The other direction: stream b of the mixed set is the block itself if stored[b] (and must then be lengths[b] long),
    else decode(stream, length, b) gives the block -> all blocks back to back."""
    payload = rcx._np_u8(payload)
    offsets = np.asarray(offsets, dtype=np.uint64)
    out = []
    for b, length in enumerate(np.asarray(lengths, dtype=np.uint64)):
        stream = payload[int(offsets[b]): int(offsets[b + 1])]
        if stored is not None and stored[b]:
            if len(stream) != int(length):
                raise ValueError(f"stored block {b} is not as long as its output")
            out.append(stream)
        else:
            out.append(rcx._np_u8(decode(stream, int(length), b)))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def _flags(stored):
    return None if stored is None else np.ascontiguousarray(np.asarray(stored) != 0, dtype=np.uint8)


def mix_device(ctx, src, block: int, comp, comp_size: int, comp_offsets, gain: int, dst, offsets, stored, stream=None, dst_cap: int | None = None) -> None:
    """Behind ctx.encode_blocks_device(src, block, comp, comp_offsets): src, comp, dst uint8 cuda tensors, comp_offsets and
    offsets int64 cuda tensors [nblocks + 1], stored a uint8 cuda tensor [nblocks].  Enqueues only."""
    n = src.numel()
    if rcx.MIN_BLOCK <= block <= rcx.MAX_BLOCK:
        nblocks = rcx.block_count(n, block)
        if offsets.numel() < nblocks + 1 or comp_offsets.numel() < nblocks + 1 or stored.numel() < nblocks:
            raise ValueError("the tables need nblocks + 1 entries and the flags nblocks")
    st = lib().rcx_stored_mix_device(ctx._h, src.data_ptr(), n, block, comp.data_ptr(), comp_size, comp_offsets.data_ptr(), gain, dst.data_ptr(),
                                     dst.numel() if dst_cap is None else dst_cap, offsets.data_ptr(), stored.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, "rcx_stored_mix_device")


def decode_device(ctx, comp, comp_size: int, comp_offsets, stored, dst_offsets, out, pick=None, coder: int = rcx.CODER_ADAPTIVE, stream=None) -> None:
    """ctx.decode_items_device with the HOST table `stored` (one entry a stream, or None): a picked stream whose entry is
    set is copied, every other one decoded.  Enqueues only."""
    doffs = np.ascontiguousarray(dst_offsets, dtype=np.uint64)
    p = None if pick is None else np.ascontiguousarray(pick, dtype=np.uint64)
    if p is not None and len(p) != len(doffs) - 1:
        raise ValueError("dst_offsets needs npick+1 entries")
    f = _flags(stored)
    if f is not None and len(f) != comp_offsets.numel() - 1:
        raise ValueError("one flag per stream")
    st = lib().rcx_stored_decode_device(ctx._h, coder, comp.data_ptr(), comp_size, comp_offsets.data_ptr(), comp_offsets.numel() - 1,
                                        None if f is None else f.ctypes.data, None if p is None else p.ctypes.data, len(doffs) - 1, doffs.ctypes.data,
                                        out.data_ptr(), ctx._stream_handle(stream))
    rcx._check(st, "rcx_stored_decode_device")


def mix(ctx, data, block: int, payload, offsets, gain: int = 0):
    """Host buffers -> (mixed payload uint8, its offsets uint64 [nblocks + 1], flags uint8 [nblocks])."""
    src, comp = rcx._np_u8(data), rcx._np_u8(payload)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    nblocks = rcx.block_count(len(src), block) if rcx.MIN_BLOCK <= block <= rcx.MAX_BLOCK else 0
    if len(offs) != nblocks + 1:
        raise ValueError("one stream per block")
    dst = np.empty(max(len(src), 1), dtype=np.uint8)
    mixed, flags = np.zeros(nblocks + 1, dtype=np.uint64), np.zeros(nblocks, dtype=np.uint8)
    size = C.c_uint64()
    st = lib().rcx_stored_mix(ctx._h, src.ctypes.data, len(src), block, comp.ctypes.data, len(comp), offs.ctypes.data, gain, dst.ctypes.data, len(src),
                              C.byref(size), mixed.ctypes.data, flags.ctypes.data)
    rcx._check(st, "rcx_stored_mix")
    return dst[: size.value], mixed, flags


def decode(ctx, payload, comp_offsets, stored, lengths, pick=None, coder: int = rcx.CODER_ADAPTIVE) -> list:
    """ctx.decode_items with the table: lengths are the decoded lengths of EVERY stream -> the list of the picked streams'
    bytes (all, if pick is None)."""
    comp = rcx._np_u8(payload)
    coffs = np.ascontiguousarray(comp_offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint64)
    f = _flags(stored)
    if len(lengths) != len(coffs) - 1 or (f is not None and len(f) != len(lengths)):
        raise ValueError("one length and one flag per stream")
    p = None if pick is None else np.ascontiguousarray(pick, dtype=np.uint64)
    if p is not None and len(p) and int(p.max()) >= len(lengths):
        raise rcx.RcxError(rcx.E_ARG, "stored.decode: pick")
    doffs = rcx.item_offsets(lengths if p is None else lengths[p.astype(np.int64)])
    out = np.empty(max(int(doffs[-1]), 1), dtype=np.uint8)
    st = lib().rcx_stored_decode(ctx._h, coder, comp.ctypes.data, len(comp), coffs.ctypes.data, len(coffs) - 1, None if f is None else f.ctypes.data,
                                 None if p is None else p.ctypes.data, len(doffs) - 1, doffs.ctypes.data, out.ctypes.data, int(doffs[-1]))
    rcx._check(st, "rcx_stored_decode")
    return [out[int(doffs[k]): int(doffs[k + 1])] for k in range(len(doffs) - 1)]
