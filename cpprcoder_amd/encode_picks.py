"""ctypes binding of include/rcx_encode_picks.h: item encode whose tables -- where the items lie, how long they are, how many are
meant -- lie in device memory.  The call plans on the GPU and only enqueues, so it can be captured in a graph, in front of
picks.decode_device if wanted, and replayed against tables that another kernel rewrites between the replays.

    entry k < min(count, max_items):   src[src_at[k] : src_at[k] + src_len[k]]  ->  stream k of a set of max_items streams

What is checked moves to the device with the tables: a bad entry is skipped and latched, every other entry is unaffected
(include/rcx_encode_picks.h has the contract in full).  plan_numpy is the planner's rules in numpy -- which entries are valid,
the length class of each, the layout of the work order in units of 64 entries with the stride and the slot base of every unit,
what is latched and at which position -- and scratch_formula the header's closed formula; they are the mirror the tests hold
the kernels and the library to.  The calls themselves are host plumbing like picks.py: every device table is a torch cuda
tensor, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .picks import CODED_BINS, PLAN_THREADS, _bytes, _table, bin_of as _pick_bin  # noqa: F401  (the planner's pieces are shared)

# every symbol include/rcx_encode_picks.h declares
EXPORTS = ("rcx_encode_picks_reserve", "rcx_encode_picks_scratch_bytes", "rcx_encode_picks_device", "rcx_encode_picks")

MAX_ITEMS = 0x7FFFFFFF
UNIT = 64                       # work positions of a unit: one stride, one slot base
CLASSES = 21                    # RCX_EPICK_CLASSES: uppers 2^24 (as MAX_BLOCK), 2^23, ... 16, longest first
PAD = UNIT * (CLASSES + 1)      # RCX_EPICK_PAD: work positions beyond max_items
RANS_MODEL_BYTES = 776 * 4      # RCX_RANS_MODEL_DW words per work position of the one-state rANS coder

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_encode_picks.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.rcx_encode_picks_reserve.restype, L.rcx_encode_picks_reserve.argtypes = i32, [vp, i32, u64, u32, u64]
        L.rcx_encode_picks_scratch_bytes.restype, L.rcx_encode_picks_scratch_bytes.argtypes = u64, [i32, u64, u32, u64]
        L.rcx_encode_picks_device.restype = i32  # ctx, coder, src, cap, src_at, src_len, count, max_items, max_len, max_bytes, dst, cap, offsets, stream
        L.rcx_encode_picks_device.argtypes = [vp, i32, vp, u64, vp, vp, vp, u64, u32, u64, vp, u64, vp, vp]
        L.rcx_encode_picks.restype = i32  # ctx, coder, src, cap, src_at, src_len, nitems, max_len, dst, cap, dst_size, offsets
        L.rcx_encode_picks.argtypes = [vp, i32, vp, u64, vp, vp, u64, u32, vp, u64, vp, vp]
        _ready = True
    return L


# ---- the planner's rules, in numpy -----------------------------------------------------------------------------------------
def class_upper(k: int) -> int:
    """The upper length of class k (0 = the longest): what its slots are sized for."""
    return min(1 << (24 - k), rcx.MAX_BLOCK)


def class_of(length: int) -> int:
    """The class of an entry of 1 .. MAX_BLOCK bytes: the power of two at or above its length, at least 16."""
    length = int(length)
    if not 1 <= length <= rcx.MAX_BLOCK:
        raise ValueError("an entry has 1 .. MAX_BLOCK bytes")
    return 24 - max((length - 1).bit_length(), 4)


def bin_of(length: int) -> int:
    """The bin of an entry in work order: picks.bin_of of length - 1 (0: the last bin), so that no bin spans two classes --
    a class is (U / 2, U], and U and U + 1 would share a bin of picks.bin_of above 512."""
    length = int(length)
    if not 1 <= length <= rcx.MAX_BLOCK:
        raise ValueError("an entry has 1 .. MAX_BLOCK bytes")
    return CODED_BINS - 1 if length == 1 else _pick_bin(length - 1)


def slots_bound(max_items: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE) -> int:
    """What the slots of at most max_items entries of max_bytes bytes between them can take, each in its class."""
    rans = coder in (rcx.CODER_RANS, rcx.CODER_RANS8)
    return 4 * max_bytes + 1152 * max_items if rans else 3 * max_bytes + 2112 * max_items


def scratch_formula(max_items: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE) -> int:
    """The formula of include/rcx_encode_picks.h for rcx_encode_picks_scratch_bytes (max_items > 0, good arguments)."""
    P = max_items + PAD
    b = 20 * P + 16 + 8 * max_items + (2 * CODED_BINS + 4) * 4 + slots_bound(max_items, max_bytes, coder) + 256 + 2 * 4 * (P + 1)
    if coder in (rcx.CODER_RANS, rcx.CODER_RANS8):
        b += 4 * (P + 1)
    if coder == rcx.CODER_RANS:
        b += RANS_MODEL_BYTES * P
    return b


def plan_numpy(src_at, src_len, count: int, max_len: int, src_cap: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE):
    """What the planner of rcx_encode_picks_device decides for these tables (max_items = len(src_len)) -> dict:
        count       min(count, max_items), how many entries are read
        valid       bool[max_items]: the entry is encoded if the total fits (not meant, empty and skipped entries: False)
        klass       int64[max_items]: the valid entry's class, 0 = the longest, -1 without one
        bins        int64[max_items]: its bin in work order, -1 without one
        total       the valid entries' bytes;  over: total > max_bytes -- nothing is encoded, every offset is 0
        class_first, class_count   int64[CLASSES]: the class's first work position (a multiple of 64) and its entries
        positions   the work positions laid out, holes included (a multiple of 64; 0 if over)
        units       [(class, stride, slot base, live entries)] per unit of 64 positions, in work order
        slots_bytes the slot memory the layout uses
        status      what rcx_ctx_sync_status returns if nothing else fails: OK, E_CORRUPT or E_CAPACITY
        position    the lowest failing position, None without a failure
    Entries at or past the count are not read: they may hold anything."""
    src_at, src_len = np.asarray(src_at, dtype=np.uint64), np.asarray(src_len, dtype=np.uint64)
    max_items = len(src_len)
    if len(src_at) != max_items:
        raise ValueError("one position and one length per entry")
    meant = min(int(count), max_items)
    valid = np.zeros(max_items, dtype=bool)
    klass = np.full(max_items, -1, dtype=np.int64)
    bins = np.full(max_items, -1, dtype=np.int64)
    corrupt, capacity = [], []
    if int(count) > max_items:
        capacity.append(max_items)
    total = 0
    for k in range(meant):
        at, length = int(src_at[k]), int(src_len[k])
        if length == 0:
            continue
        if length > max_len:
            corrupt.append(k)
        elif at > src_cap or length > src_cap - at:
            capacity.append(k)
        else:
            valid[k], klass[k], bins[k] = True, class_of(length), bin_of(length)
            total += length
    over = total > max_bytes
    if over:
        capacity.append(meant)
    class_count = np.array([int(np.sum(klass == c)) for c in range(CLASSES)], dtype=np.int64)
    class_first = np.zeros(CLASSES, dtype=np.int64)
    units, pos, base = [], 0, 0
    for c in range(CLASSES):
        class_first[c] = pos
        stride, n = rcx.block_bound(class_upper(c), coder), int(class_count[c])
        for u in range(-(-n // UNIT)):
            units.append((c, stride, base + u * UNIT * stride, min(UNIT, n - u * UNIT)))
        pos += -(-n // UNIT) * UNIT
        base += n * stride
    failing = corrupt + capacity
    return {"count": meant, "valid": valid, "klass": klass, "bins": bins, "total": total, "over": over, "class_first": class_first,
            "class_count": class_count, "positions": 0 if over else pos, "units": [] if over else units, "slots_bytes": 0 if over else base,
            "status": rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if capacity else rcx.OK, "position": min(failing) if failing else None}


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(max_items: int, max_len: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE) -> int:
    """rcx_encode_picks_scratch_bytes: what Context.scratch_bytes() reports for a fresh context after reserve(); 0 for bad arguments."""
    if not (0 <= max_items < 1 << 64 and 0 <= max_len < 1 << 32 and 0 <= max_bytes < 1 << 64):
        return 0
    return int(lib().rcx_encode_picks_scratch_bytes(coder, max_items, max_len, max_bytes))


def reserve(ctx, max_items: int, max_len: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE) -> None:
    """rcx_encode_picks_reserve: after it, encode_device with at most max_items entries of at most max_len bytes and max_bytes
    between them allocates nothing and is launches only."""
    rcx._check(lib().rcx_encode_picks_reserve(ctx._h, coder, max_items, max_len, max_bytes), "rcx_encode_picks_reserve")


def dst_bound(max_items: int, max_bytes: int, coder: int = rcx.CODER_ADAPTIVE) -> int:
    """A dst_cap that is always enough: the sum of rcx_block_bound_for over entries of max_bytes bytes between them is at most
    this (the range coders: len * (1 + 1/32 + 1/8) + 2063 an entry; the rANS coders: 2 * len + 1111)."""
    if coder in (rcx.CODER_RANS, rcx.CODER_RANS8):
        return 2 * max_bytes + 1112 * max_items
    return max_bytes + -(-5 * max_bytes // 32) + 2064 * max_items


def encode_device(ctx, src, src_at, src_len, count, dst, comp_offsets, max_len: int, max_bytes: int, max_items: int | None = None,
                  coder: int = rcx.CODER_ADAPTIVE, stream=None, src_cap: int | None = None, dst_cap: int | None = None) -> None:
    """src, dst: uint8 cuda tensors; src_at, src_len: int64 cuda tensors [>= max_items] (max_items = src_len.numel() if None);
    count: an int64 cuda tensor of one entry; comp_offsets: an int64 cuda tensor [>= max_items + 1], written whole.  Enqueues
    only; after reserve() it may be captured in a graph."""
    max_items = src_len.numel() if max_items is None else int(max_items)
    if not 0 <= max_items <= MAX_ITEMS:
        raise ValueError("max_items is 0 .. 2^31 - 1")
    src_cap = src.numel() if src_cap is None else int(src_cap)
    dst_cap = dst.numel() if dst_cap is None else int(dst_cap)
    args = (_bytes(src, src_cap, "src"), src_cap, _table(src_at, max_items, "src_at"), _table(src_len, max_items, "src_len"), _table(count, 1, "count"),
            max_items, max_len, max_bytes, _bytes(dst, dst_cap, "dst"), dst_cap, _table(comp_offsets, max_items + 1, "comp_offsets"))
    rcx._check(lib().rcx_encode_picks_device(ctx._h, coder, *args, ctx._stream_handle(stream)), "rcx_encode_picks_device")


def encode(ctx, src, src_at, src_len, max_len: int, coder: int = rcx.CODER_ADAPTIVE, dst_cap: int | None = None):
    """rcx_encode_picks on host buffers: every entry is meant -> (payload uint8, comp_offsets uint64[nitems + 1], the latched
    status: OK, E_CORRUPT or E_CAPACITY).  The good entries' streams are there also behind a latched failure."""
    data = rcx._np_u8(src)
    at, ln = (np.ascontiguousarray(x, dtype=np.uint64) for x in (src_at, src_len))
    if len(at) != len(ln):
        raise ValueError("one position and one length per entry")
    good = (ln <= max_len) & (at <= len(data)) & (ln <= np.uint64(len(data)) - np.minimum(at, np.uint64(len(data))))
    cap = dst_bound(len(ln), int(ln[good].sum()), coder) + 16 if dst_cap is None else int(dst_cap)
    dst = np.zeros(max(cap, 16), dtype=np.uint8)
    offs = np.zeros(len(ln) + 1, dtype=np.uint64)
    size = C.c_uint64()
    st = lib().rcx_encode_picks(ctx._h, coder, data.ctypes.data, len(data), at.ctypes.data, ln.ctypes.data, len(ln), max_len, dst.ctypes.data, cap,
                                C.byref(size), offs.ctypes.data)
    if st in (rcx.E_ARG, rcx.E_HIP, rcx.E_NOMEM):
        raise rcx.RcxError(st, "rcx_encode_picks")
    return dst[: min(int(size.value), cap)], offs, st


# ---- the container's side: reached as container.pack_items_device and container.PackedItems (container.__getattr__) ------------
class PackedItems:
    """What pack_items_device leaves on the device: max_items streams in d_payload at d_offsets (the streams at or behind the
    count are empty), the caller's tables of lengths and the count beside them.  It is an OpenItems that was never a file:
    decode_into is the same call, and to_bytes() makes the file."""

    def __init__(self, ctx, coder, d_src_len, d_count, max_items, max_len, d_payload, d_offsets):
        from . import picks
        self.ctx, self.coder, self.nitems, self.max_len = ctx, coder, max_items, max_len
        self.d_lengths, self.d_count, self.d_payload, self.d_offsets = d_src_len, d_count, d_payload, d_offsets
        self.payload_size = d_payload.numel()
        self._picks = picks

    def reserve(self, max_pick: int) -> None:
        """The scratch of decode_into calls with at most max_pick entries: after it they allocate nothing in the context."""
        self._picks.reserve(self.ctx, max_pick, self.max_len, self.coder)

    def decode_into(self, d_pick, d_dst_at, d_count, d_dst, max_pick: int | None = None, stream=None) -> None:
        """OpenItems.decode_into over the streams where the encode call left them: entry k < d_count[0]: item d_pick[k] ->
        d_dst[d_dst_at[k] : + its length].  Nothing is downloaded: the lengths and the number of items are read on the device (an
        entry that names no item gets length 1 and a stream past the set, so that the call skips and latches it)."""
        import torch
        max_pick = d_pick.numel() if max_pick is None else int(max_pick)
        p = d_pick[:max_pick]
        inside = (p >= 0) & (p < torch.clamp(self.d_count[0], 0, self.nitems))
        d_len = torch.where(inside, self.d_lengths[torch.clamp(p, 0, max(self.nitems - 1, 0))], torch.ones_like(p))
        p = torch.where(inside, p, torch.full_like(p, self.nitems))
        self._picks.decode_device(self.ctx, self.d_payload, self.payload_size, self.d_offsets, p, d_dst_at, d_len, d_count, d_dst, self.max_len,
                                  max_pick=max_pick, coder=self.coder, stream=stream)

    def to_bytes(self) -> bytes:
        """Synchronises (a latched failure of the encode call is raised), downloads, and writes the RCXI container that pack_items
        writes for the same items, without checksums."""
        self.ctx.sync_status()
        n = min(max(int(self.d_count[0]), 0), self.nitems)
        offsets = self.d_offsets[: n + 1].cpu().numpy().astype(np.uint64)
        lengths = self.d_lengths[:n].cpu().numpy().astype(np.uint64)
        from .layout import item_header_bytes
        return item_header_bytes(self.coder, lengths, offsets) + self.d_payload[: int(offsets[-1])].cpu().numpy().tobytes()


def pack_items_device(ctx, d_src, d_src_at, d_src_len, d_count, max_items: int, max_len: int, max_bytes: int, coder: int = 0, stream=None) -> PackedItems:
    """Items that device code chose -- entry k < d_count[0] is d_src[d_src_at[k] : + d_src_len[k]] (int64 cuda tensors [>= max_items],
    d_count one entry) -- encoded where they lie (include/rcx_encode_picks.h); reached as container.pack_items_device.  Allocates the output once,
    enqueues the call and returns: no download, no synchronisation.  -> PackedItems over the device-resident streams.  No checksums."""
    import torch
    _bytes(d_src, 0, "d_src")  # (host tensors are refused before anything is allocated)
    for t, least, what in ((d_src_at, max_items, "d_src_at"), (d_src_len, max_items, "d_src_len"), (d_count, 1, "d_count")):
        _table(t, least, what)
    d_payload = torch.empty(max(dst_bound(max_items, max_bytes, coder), 16), dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(max_items + 1, dtype=torch.int64, device="cuda")
    encode_device(ctx, d_src, d_src_at, d_src_len, d_count, d_payload, d_offsets, max_len, max_bytes, max_items=max_items, coder=coder,
                               stream=stream)
    return PackedItems(ctx, coder, d_src_len, d_count, max_items, max_len, d_payload, d_offsets)
