"""ctypes binding of include/rcx_stored_items.h: stored items -- the mix of stored.py behind the ITEM encode call.  An item whose
stream did not shrink is kept as its raw bytes and decoded by copy, so a set of item streams never exceeds its items.

The rule is stored.is_stored with the item in the block's place, and one more: an item of length 0 has no stream and is never
stored.  include/rcx_stored_items.h has the contract in full, and a worked example.  Decode needs no call of its own:
stored.decode_device / stored.decode are in item geometry.

mix_items_numpy is the rule in numpy -- the mirror the tests hold the kernels to.  The calls themselves are host plumbing like
rcx.py: the signatures are set on rcx.lib()'s handle, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .stored import GAIN_MAX, GAIN_ONE, gain_q16, is_stored  # noqa: F401 (one rule for blocks and items)

# every symbol include/rcx_stored_items.h declares
EXPORTS = ("rcx_stored_mix_items_device", "rcx_stored_mix_items")

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the two calls of include/rcx_stored_items.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.rcx_stored_mix_items_device.restype, L.rcx_stored_mix_items_device.argtypes = i32, [vp, vp, vp, u64, vp, u64, vp, u32, vp, u64, vp, vp, vp]
        L.rcx_stored_mix_items.restype, L.rcx_stored_mix_items.argtypes = i32, [vp, vp, vp, u64, vp, u64, vp, u32, vp, u64, vp, vp, vp]
        _ready = True
    return L


# ---- the rule, in numpy ------------------------------------------------------------------------------------------------------
def mix_items_numpy(src, src_offsets, payload, offsets, gain: int = 0):
    """What rcx_stored_mix_items writes: item i is src[src_offsets[i] : src_offsets[i + 1]], its stream
    payload[offsets[i] : offsets[i + 1]] -> (mixed payload uint8, its offsets uint64 [nitems + 1], flags uint8 [nitems]).
    An empty item is never stored, and its entry of `offsets` is not looked at."""
    src, payload = rcx._np_u8(src), rcx._np_u8(payload)
    soffs = np.asarray(src_offsets, dtype=np.uint64).astype(np.int64)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    if len(soffs) < 1 or len(offsets) != len(soffs):
        raise ValueError("one stream per item, and nitems + 1 offsets in both tables")
    lengths = np.diff(soffs)
    if np.any(lengths < 0) or (len(lengths) and int(soffs[-1]) > len(src)):
        raise ValueError("the items' offsets decrease or run past the buffer")
    live = lengths > 0
    coded = np.where(live, np.diff(offsets), 0)
    if np.any(coded < 0) or (live.any() and int(offsets[1:][live].max()) > len(payload)):
        raise ValueError("the streams' offsets decrease or run past the payload")
    flags = np.asarray(is_stored(coded, lengths, gain), dtype=bool).reshape(len(lengths)) & live
    parts = []
    for i in range(len(lengths)):
        if not live[i]:
            parts.append(src[:0])
        elif flags[i]:
            parts.append(src[int(soffs[i]): int(soffs[i + 1])])
        else:
            parts.append(payload[int(offsets[i]): int(offsets[i + 1])])
    mixed = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=mixed[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), mixed, flags.astype(np.uint8)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def mix_items_device(ctx, src, src_offsets, comp, comp_size: int, comp_offsets, gain: int, dst, offsets, stored, stream=None,
                     dst_cap: int | None = None) -> None:
    """Behind ctx.encode_items_device(src, src_offsets, comp, comp_offsets): src, comp, dst uint8 cuda tensors, src_offsets the
    HOST table of the items, comp_offsets and offsets int64 cuda tensors [nitems + 1], stored a uint8 cuda tensor [nitems].
    Enqueues only; cannot be captured."""
    soffs = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    nitems = len(soffs) - 1
    if nitems < 0 or offsets.numel() < nitems + 1 or comp_offsets.numel() < nitems + 1 or stored.numel() < nitems:
        raise ValueError("the tables need nitems + 1 entries and the flags nitems")
    if nitems and int(soffs[-1]) > src.numel():
        raise ValueError("the offsets run past src")
    st = lib().rcx_stored_mix_items_device(ctx._h, src.data_ptr(), soffs.ctypes.data, nitems, comp.data_ptr(), comp_size, comp_offsets.data_ptr(), gain,
                                           dst.data_ptr(), dst.numel() if dst_cap is None else dst_cap, offsets.data_ptr(), stored.data_ptr(),
                                           ctx._stream_handle(stream))
    rcx._check(st, "rcx_stored_mix_items_device")


def mix_items(ctx, data, src_offsets, payload, offsets, gain: int = 0):
    """Host buffers -> (mixed payload uint8, its offsets uint64 [nitems + 1], flags uint8 [nitems])."""
    src, comp = rcx._np_u8(data), rcx._np_u8(payload)
    soffs = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    nitems = len(soffs) - 1
    if nitems < 0 or len(offs) != nitems + 1:
        raise ValueError("one stream per item, and nitems + 1 offsets in both tables")
    if nitems and int(soffs[-1]) > len(src):
        raise ValueError("the offsets run past the buffer")
    cap = int(soffs[-1] - soffs[0]) if nitems else 0
    dst = np.empty(max(cap, 1), dtype=np.uint8)
    mixed, flags = np.zeros(nitems + 1, dtype=np.uint64), np.zeros(nitems, dtype=np.uint8)
    size = C.c_uint64()
    st = lib().rcx_stored_mix_items(ctx._h, src.ctypes.data, soffs.ctypes.data, nitems, comp.ctypes.data, len(comp), offs.ctypes.data, gain,
                                    dst.ctypes.data, cap, C.byref(size), mixed.ctypes.data, flags.ctypes.data)
    rcx._check(st, "rcx_stored_mix_items")
    return dst[: size.value], mixed, flags
