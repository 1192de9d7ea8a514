"""ctypes binding of include/rcx_picks.h: item decode whose tables -- which streams, where their bytes go, how many entries are
meant, which streams are stored -- lie in device memory.  The call plans on the GPU and only enqueues, so it can be captured
in a graph and replayed against tables that another kernel rewrites between the replays.

    entry k < min(count, max_pick):   stream pick[k]  ->  dst[dst_at[k] : dst_at[k] + dst_len[k]]

What is checked moves to the device with the tables: a bad entry is skipped and latched, every other entry is unaffected
(include/rcx_picks.h has the contract in full).  plan_numpy is those rules in numpy -- which entries are valid, which are
copied, what is latched and at which position -- and bin_of the planner's work order; they are the mirror the tests hold the
kernels to.  The calls themselves are host plumbing like rcx.py: the signatures are set on rcx.lib()'s handle, every device
table is a torch cuda tensor, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx

# every symbol include/rcx_picks.h declares
EXPORTS = ("rcx_picks_reserve", "rcx_picks_scratch_bytes", "rcx_decode_picks_device", "rcx_decode_picks")

MAX_PICK = 0x7FFFFFFF
COPY_SHORT = 1024            # RCX_COPY_SHORT: a stored pick above this many bytes is a workgroup's, else a wave's
EXACT = 512                  # RCX_PICK_EXACT: lengths below this have a bin each
CODED_BINS = EXACT + (24 - 9) * 256  # RCX_PICK_CODED_BINS
BINS = CODED_BINS + 2        # + stored long, stored short
PLAN_THREADS = 256           # RCX_PICK_THREADS: entries a workgroup of the planner takes at a go
NONE, CODED, STORED_LONG, STORED_SHORT = 0, 1, 2, 3  # an entry's route

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_picks.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.rcx_picks_reserve.restype, L.rcx_picks_reserve.argtypes = i32, [vp, i32, u64, u32]
        L.rcx_picks_scratch_bytes.restype, L.rcx_picks_scratch_bytes.argtypes = u64, [i32, u64, u32]
        L.rcx_decode_picks_device.restype = i32
        L.rcx_decode_picks_device.argtypes = [vp, i32, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, u32, vp, u64, vp]
        L.rcx_decode_picks.restype = i32
        L.rcx_decode_picks.argtypes = [vp, i32, vp, u64, vp, u64, vp, vp, vp, vp, u64, u32, vp, u64]
        _ready = True
    return L


# ---- the planner's rules, in numpy -----------------------------------------------------------------------------------------
def len_bin(length: int, top_bits: int) -> int:
    """rcx_len_bin, the one bin rule: the bin of `length` bytes, 1 <= length < 2^top_bits, in work order: ascending bins are
    descending lengths.  A length below 512 has a bin of its own; above, the bin is the length's leading one and the eight bits
    behind it."""
    length = int(length)
    if not 1 <= length < 1 << top_bits:
        raise ValueError(f"an entry has 1 .. 2^{top_bits} - 1 bytes")
    up = length
    if length >= EXACT:
        e = length.bit_length() - 1
        up = EXACT + (e - 9) * 256 + ((length >> (e - 8)) & 255)
    return EXACT + (top_bits - 9) * 256 - 1 - up


def bin_of(length: int) -> int:
    """The bin of a coded pick of `length` bytes, 1 <= length < 2^24: len_bin among CODED_BINS."""
    return len_bin(length, 24)


def plan_numpy(pick, dst_at, dst_len, count: int, max_len: int, nstreams: int, dst_cap: int, stored=None, comp_offsets=None, comp_size: int | None = None):
    """What the planner of rcx_decode_picks_device decides for these tables (max_pick = len(pick)) -> dict:
        count     min(count, max_pick), how many entries are read
        route     uint8[max_pick]: NONE (not meant, empty or skipped), CODED, STORED_LONG or STORED_SHORT
        bins      int64[max_pick]: the entry's bin in work order, -1 without a route
        status    what rcx_ctx_sync_status returns if every stream decodes: OK, E_CORRUPT or E_CAPACITY
        position  the lowest failing position, None without a failure
    Entries at or past the count are not read: they may hold anything."""
    pick = np.asarray(pick, dtype=np.uint64)
    dst_at, dst_len = np.asarray(dst_at, dtype=np.uint64), np.asarray(dst_len, dtype=np.uint64)
    max_pick = len(pick)
    if len(dst_at) != max_pick or len(dst_len) != max_pick:
        raise ValueError("one destination and one length per pick")
    if stored is not None:
        if comp_offsets is None or comp_size is None:
            raise ValueError("flags need the streams' table and size")
        stored = np.asarray(stored) != 0
        offs = np.asarray(comp_offsets, dtype=np.uint64)
        if len(stored) != nstreams or len(offs) != nstreams + 1:
            raise ValueError("one flag a stream, and nstreams + 1 offsets")
    meant = min(int(count), max_pick)
    route = np.zeros(max_pick, dtype=np.uint8)
    bins = np.full(max_pick, -1, dtype=np.int64)
    corrupt, capacity = [], []
    if int(count) > max_pick:
        capacity.append(max_pick)
    for k in range(meant):
        st, at, length = int(pick[k]), int(dst_at[k]), int(dst_len[k])
        if length == 0:
            continue
        if st >= nstreams or length > max_len:
            corrupt.append(k)
        elif at + length > dst_cap:
            capacity.append(k)
        elif stored is not None and stored[st]:
            s0, s1 = int(offs[st]), int(offs[st + 1])
            if s1 >= s0 and s1 <= comp_size and s1 - s0 == length:
                route[k] = STORED_LONG if length > COPY_SHORT else STORED_SHORT
                bins[k] = CODED_BINS + (0 if length > COPY_SHORT else 1)
            else:
                corrupt.append(k)
        else:
            route[k] = CODED
            bins[k] = bin_of(length)
    failing = corrupt + capacity
    return {"count": meant, "route": route, "bins": bins, "status": rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if capacity else rcx.OK,
            "position": min(failing) if failing else None}


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(max_pick: int, max_len: int, coder: int = rcx.CODER_ADAPTIVE) -> int:
    """rcx_picks_scratch_bytes: what Context.scratch_bytes() reports for a fresh context after reserve(); 0 for bad arguments."""
    if not (0 <= max_pick < 1 << 64 and 0 <= max_len < 1 << 32):
        return 0
    return int(lib().rcx_picks_scratch_bytes(coder, max_pick, max_len))


def reserve(ctx, max_pick: int, max_len: int, coder: int = rcx.CODER_ADAPTIVE) -> None:
    """rcx_picks_reserve: after it, decode_device with at most max_pick entries of at most max_len bytes allocates nothing."""
    rcx._check(lib().rcx_picks_reserve(ctx._h, coder, max_pick, max_len), "rcx_picks_reserve")


def _table(t, least: int, what: str):
    """A device table of 8-byte integers with `least` entries at least."""
    if not getattr(t, "is_cuda", False):
        raise ValueError(f"{what} is a torch cuda tensor: the call reads it on the device")
    if t.element_size() != 8 or t.is_floating_point() or not t.is_contiguous():
        raise ValueError(f"{what} holds contiguous 64-bit integers")
    if t.numel() < least:
        raise ValueError(f"{what} needs {least} entries")
    return t.data_ptr()


def _bytes(t, least: int, what: str):
    if not getattr(t, "is_cuda", False):
        raise ValueError(f"{what} is a torch cuda tensor: the call reads it on the device")
    if t.element_size() != 1 or not t.is_contiguous():
        raise ValueError(f"{what} holds contiguous bytes")
    if t.numel() < least:
        raise ValueError(f"{what} needs {least} bytes")
    return t.data_ptr()


def decode_device(ctx, comp, comp_size: int, comp_offsets, pick, dst_at, dst_len, count, out, max_len: int, max_pick: int | None = None, stored=None,
                  coder: int = rcx.CODER_ADAPTIVE, stream=None, dst_cap: int | None = None) -> None:
    """comp, out: uint8 cuda tensors; comp_offsets: int64 cuda tensor [nstreams + 1]; pick, dst_at, dst_len: int64 cuda tensors
    [>= max_pick] (max_pick = pick.numel() if None); count: int64 cuda tensor of one entry; stored: uint8 cuda tensor [nstreams]
    or None.  Enqueues only; after reserve() it may be captured in a graph."""
    max_pick = pick.numel() if max_pick is None else int(max_pick)
    if not 0 <= max_pick <= MAX_PICK:
        raise ValueError("max_pick is 0 .. 2^31 - 1")
    nstreams = comp_offsets.numel() - 1
    if nstreams < 0:
        raise ValueError("comp_offsets needs nstreams + 1 entries")
    args = (_bytes(comp, comp_size, "comp"), comp_size, _table(comp_offsets, nstreams + 1, "comp_offsets"), nstreams,
            None if stored is None else _bytes(stored, nstreams, "stored"), _table(pick, max_pick, "pick"), _table(dst_at, max_pick, "dst_at"),
            _table(dst_len, max_pick, "dst_len"), _table(count, 1, "count"), max_pick, max_len, _bytes(out, 0 if dst_cap is None else dst_cap, "out"),
            out.numel() if dst_cap is None else dst_cap)
    rcx._check(lib().rcx_decode_picks_device(ctx._h, coder, *args, ctx._stream_handle(stream)), "rcx_decode_picks_device")


def decode(ctx, payload, comp_offsets, pick, dst_at, dst_len, max_len: int, dst: np.ndarray, stored=None, coder: int = rcx.CODER_ADAPTIVE):
    """rcx_decode_picks on host buffers: every entry is meant; dst (uint8, written in place) -> the latched status (OK, E_CORRUPT or
    E_CAPACITY).  The good entries are written also behind a latched failure."""
    comp = rcx._np_u8(payload)
    coffs = np.ascontiguousarray(comp_offsets, dtype=np.uint64)
    p, at, ln = (np.ascontiguousarray(x, dtype=np.uint64) for x in (pick, dst_at, dst_len))
    if len(at) != len(p) or len(ln) != len(p):
        raise ValueError("one destination and one length per pick")
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
        raise ValueError("dst is a writable contiguous uint8 array")
    f = None if stored is None else np.ascontiguousarray(np.asarray(stored) != 0, dtype=np.uint8)
    if f is not None and len(f) != len(coffs) - 1:
        raise ValueError("one flag per stream")
    st = lib().rcx_decode_picks(ctx._h, coder, comp.ctypes.data, len(comp), coffs.ctypes.data, len(coffs) - 1, None if f is None else f.ctypes.data,
                                p.ctypes.data, at.ctypes.data, ln.ctypes.data, len(p), max_len, dst.ctypes.data, len(dst))
    if st in (rcx.E_ARG, rcx.E_HIP, rcx.E_NOMEM):
        raise rcx.RcxError(st, "rcx_decode_picks")
    return st
