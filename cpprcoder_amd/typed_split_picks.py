"""ctypes binding of include/rcx_typed_split_picks.h: the typed split per item whose tables -- where each item's bytes lie, where
its split text goes, its length, width and predictor, how many entries are meant -- lie in device memory.  The call plans on the
GPU and only enqueues, so it can stand in front of encode_picks.encode_device inside one captured graph.  The mirror of
typed_picks.py.

    entry k < min(count, max_pick):   split of src[src_at[k] : + len[k]]  ->  dst[dst_at[k] : + len[k]],  kept[k] = len[k]

What is checked moves to the device with the tables: a bad entry is skipped and latched (kept 0), every other entry is split, and
when the valid entries have more than max_bytes between them nothing is split (include/rcx_typed_split_picks.h has the contract
in full).  plan_numpy is those rules in numpy -- validation, the class of every entry, its place within the class, ufirst, the head
of the tables, kept, status and position; it is the mirror the tests hold the kernels to.  The calls themselves are host plumbing
like rcx.py: every device table is a torch cuda tensor, and there is no CPU fallback.

The container's side is at the end: pack_typed_items_device and PackedTypedItems, reached as container.pack_typed_items_device and
container.PackedTypedItems (container.__getattr__).
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import rcx
from .predict import ZIGZAG
from .typed_picks import (HEAD_BYTES, MAX_BLOCK, MAX_BYTES, MAX_PICK, PLAN_GRID, PLAN_THREADS, PLAN_TOP, ROW, ROW_BYTES, TYPED_STEP_ROWS, _table,  # noqa: F401
                          head_of, set_tables)  # (the planner's shapes and its rendering of a set are shared)

# every symbol include/rcx_typed_split_picks.h declares
EXPORTS = ("rcx_typed_split_picks_reserve", "rcx_typed_split_picks_scratch_bytes", "rcx_typed_split_picks_device", "rcx_typed_split_picks")

CLASSES = 12         # RCX_TYPED_CLASSES: class = 3 * log2(width) + predictor; 1 and 2 stay empty (width 1 takes no predictor)
PLANES_U4 = 16       # RCX_PLANES_U4: a workgroup step is PLANES_U4 / width rows
NO_CLASS = -1

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_typed_split_picks.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_typed_split_picks_reserve.restype, L.rcx_typed_split_picks_reserve.argtypes = i32, [vp, u64, u64]
        L.rcx_typed_split_picks_scratch_bytes.restype, L.rcx_typed_split_picks_scratch_bytes.argtypes = u64, [u64, u64]
        L.rcx_typed_split_picks_device.restype = i32
        L.rcx_typed_split_picks_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u64, vp, u64, vp, vp]
        L.rcx_typed_split_picks.restype = i32
        L.rcx_typed_split_picks.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, u64, vp]
        _ready = True
    return L


# ---- the planner's rules, in numpy -----------------------------------------------------------------------------------------
def class_of(width: int, pred: int) -> int:
    """rcx_typed_class: 3 * log2(width) + predictor."""
    return 3 * {1: 0, 2: 1, 4: 2, 8: 3}[int(width)] + int(pred)


def scratch_formula(max_pick: int, max_bytes: int) -> int:
    """The formula of include/rcx_typed_split_picks.h for rcx_typed_split_picks_scratch_bytes."""
    if not (0 < max_pick <= MAX_PICK and 0 <= max_bytes <= MAX_BYTES):
        return 0
    tiles, rows = (max_pick + PLAN_THREADS - 1) // PLAN_THREADS, max_bytes // ROW_BYTES + 2 * CLASSES
    n = HEAD_BYTES + 8 * (max_pick + 1) + 16 * max_pick + 200 * tiles + 48 * tiles + 8 * max_pick + 4 * rows + 8
    return (n + 7) // 8 * 8


def head_numpy(nent, units):
    """The head of the tables from the 12 classes' entries and whole units, as rcx_typed_plan(..., scan = false) computes it ->
    dict(step_end[12], rest_end[12], ubase[13], ent_first[13], row_first[13]) of Python integers."""
    ent_first, row_first, ubase, step_end, rest_end = head_of(nent, units, TYPED_STEP_ROWS)
    return {"step_end": step_end, "rest_end": rest_end, "ubase": ubase, "ent_first": ent_first, "row_first": row_first}


def plan_numpy(src_at, dst_at, length, widths, preds, count: int, max_bytes: int, src_cap: int, dst_cap: int):
    """What the planner of rcx_typed_split_picks_device decides for these tables (max_pick = len(length)) -> dict:
        count     min(count, max_pick), how many entries are read
        valid     bool[max_pick]: the entry passed the checks (it is split unless the call overflows)
        klass     int64[max_pick]: a valid entry's class, else NO_CLASS
        place     int64[max_pick]: its entry in the planned tables -- the caller's order within the class -- else -1 (also when
                  the call overflows)
        ufirst    uint64[nent + 1]: the first whole unit of every placed entry, numbered through the classes, and the closing one
        order     int64[nent]: the entry k of the call that lies at each place
        head      head_numpy of the placed entries
        kept      uint64[max_pick]: the entry's length if it is split, else 0 -- what the call writes to d_kept
        bytes     what the valid entries have between them
        overflow  bytes > max_bytes: nothing is split
        status    what rcx_ctx_sync_status returns: OK, E_CORRUPT or E_CAPACITY
        position  the lowest failing position, None without a failure
    Entries at or past the count are not read: they may hold anything.  preds may be None: no entry has a predictor."""
    src_at, dst_at, length = (np.asarray(x, dtype=np.uint64) for x in (src_at, dst_at, length))
    widths = np.asarray(widths, dtype=np.uint8)
    max_pick = len(length)
    preds = np.zeros(max_pick, np.uint8) if preds is None else np.asarray(preds, dtype=np.uint8)
    if not (len(src_at) == len(dst_at) == len(widths) == len(preds) == max_pick):
        raise ValueError("one source, destination, length, width and predictor per entry")
    meant = min(int(count), max_pick)
    valid = np.zeros(max_pick, dtype=bool)
    klass = np.full(max_pick, NO_CLASS, dtype=np.int64)
    corrupt, capacity = [], []
    if int(count) > max_pick:
        capacity.append(max_pick)
    total = 0
    for k in range(meant):
        n, w, p, a, b = int(length[k]), int(widths[k]), int(preds[k]), int(src_at[k]), int(dst_at[k])
        if n == 0:
            continue
        if w not in (1, 2, 4, 8) or p > ZIGZAG or (w == 1 and p) or n // w + n % w > MAX_BLOCK:
            corrupt.append(k)
        elif a + n > src_cap or b + n > dst_cap:  # (Python's integers: no sum wraps)
            capacity.append(k)
        else:
            valid[k], klass[k] = True, class_of(w, p)
            total += n
    overflow = total > max_bytes
    if overflow:
        capacity.append(meant)
    placed = [] if overflow else [(int(klass[k]), int(k), int(length[k]), int(widths[k])) for k in np.flatnonzero(valid)]
    t = set_tables(placed, TYPED_STEP_ROWS)  # by class, the caller's order within it
    order, ufirst = t["entry"], t["ufirst"]
    place = np.full(max_pick, -1, dtype=np.int64)
    place[order] = np.arange(len(order))
    kept = np.where(place >= 0, length, np.uint64(0)).astype(np.uint64)
    head = {key: [int(x) for x in t[key]] for key in ("step_end", "rest_end", "ubase", "ent_first", "row_first")}
    failing = corrupt + capacity
    return {"count": meant, "valid": valid, "klass": klass, "place": place, "ufirst": ufirst, "order": order, "head": head,
            "kept": kept, "bytes": total, "overflow": overflow,
            "status": rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if capacity else rcx.OK, "position": min(failing) if failing else None}


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(max_pick: int, max_bytes: int) -> int:
    """rcx_typed_split_picks_scratch_bytes: what Context.scratch_bytes() reports for a fresh context after reserve(); 0 for bad arguments."""
    if not (0 <= max_pick < 1 << 64 and 0 <= max_bytes < 1 << 64):
        return 0
    return int(lib().rcx_typed_split_picks_scratch_bytes(max_pick, max_bytes))


def reserve(ctx, max_pick: int, max_bytes: int) -> None:
    """rcx_typed_split_picks_reserve: after it, split_device with at most max_pick entries of at most max_bytes together allocates nothing."""
    rcx._check(lib().rcx_typed_split_picks_reserve(ctx._h, max_pick, max_bytes), "rcx_typed_split_picks_reserve")


def split_device(ctx, src, src_at, dst_at, length, widths, preds, count, dst, max_bytes: int, max_pick: int | None = None, kept=None, stream=None,
                 src_cap: int | None = None, dst_cap: int | None = None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; src_at, dst_at, length: int64 cuda tensors [>= max_pick] (max_pick =
    length.numel() if None); widths, preds: uint8 cuda tensors [>= max_pick], preds may be None; count: int64 cuda tensor of one
    entry; kept: None or an int64 cuda tensor [>= max_pick], written whole.  Enqueues only; after reserve() it may be captured in a graph."""
    max_pick = length.numel() if max_pick is None else int(max_pick)
    if not 0 <= max_pick <= MAX_PICK:
        raise ValueError("max_pick is 0 .. 2^31 - 1")
    if not 0 <= max_bytes <= MAX_BYTES:
        raise ValueError("max_bytes is 0 .. 2^42")
    src_cap = src.numel() if src_cap is None else int(src_cap)
    dst_cap = dst.numel() if dst_cap is None else int(dst_cap)
    args = (_table(src, src_cap, "src", 1), src_cap, _table(src_at, max_pick, "src_at", 8), _table(dst_at, max_pick, "dst_at", 8),
            _table(length, max_pick, "length", 8), _table(widths, max_pick, "widths", 1), None if preds is None else _table(preds, max_pick, "preds", 1),
            _table(count, 1, "count", 8), max_pick, max_bytes, _table(dst, dst_cap, "dst", 1), dst_cap, None if kept is None else _table(kept, max_pick, "kept", 8))
    rcx._check(lib().rcx_typed_split_picks_device(ctx._h, *args, ctx._stream_handle(stream)), "rcx_typed_split_picks_device")


def split(ctx, src, src_at, dst_at, length, widths, preds, dst: np.ndarray):
    """rcx_typed_split_picks on host buffers: every entry is meant; dst (uint8, written in place) -> (the latched status: OK,
    E_CORRUPT or E_CAPACITY; kept uint64[npick]).  The good entries are written also behind a latched failure."""
    x = rcx._np_u8(src)
    a, b, n = (np.ascontiguousarray(t, dtype=np.uint64) for t in (src_at, dst_at, length))
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    p = None if preds is None else np.ascontiguousarray(preds, dtype=np.uint8)
    if not (len(a) == len(b) == len(w) == len(n)) or (p is not None and len(p) != len(n)):
        raise ValueError("one source, destination, length, width and predictor per entry")
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
        raise ValueError("dst is a writable contiguous uint8 array")
    kept = np.zeros(max(len(n), 1), dtype=np.uint64)
    st = lib().rcx_typed_split_picks(ctx._h, x.ctypes.data, len(x), a.ctypes.data, b.ctypes.data, n.ctypes.data, w.ctypes.data,
                                     None if p is None else p.ctypes.data, len(n), dst.ctypes.data, len(dst), kept.ctypes.data)
    if st in (rcx.E_ARG, rcx.E_HIP, rcx.E_NOMEM):
        raise rcx.RcxError(st, "rcx_typed_split_picks")
    return st, kept[: len(n)]


# ---- the container's side: reached as container.pack_typed_items_device and container.PackedTypedItems -------------------------
SLOTS = 8  # OpenTypedItems.SLOTS: table entries an item, in every one of the four calls


def compact_offsets(widths, offsets8) -> np.ndarray:
    """The stream table of 8 slots an item (uint64[8 n + 1], the empty slots' streams empty) -> the table of the container's
    sum-of-widths sub-items (uint64[nsub + 1]): item i keeps slots 8 i .. 8 i + widths[i] - 1.  The payload needs no move: an empty
    stream has no bytes, so the kept streams lie back to back already."""
    widths = np.asarray(widths, dtype=np.int64)
    offsets8 = np.asarray(offsets8, dtype=np.uint64)
    n = len(widths)
    if len(offsets8) != SLOTS * n + 1:
        raise ValueError("eight slots an item and the closing offset")
    if np.any((widths < 1) | (widths > SLOTS)):
        raise ValueError("an element is 1, 2, 4 or 8 bytes wide")
    q = np.arange(SLOTS)[None, :]
    keep = (q < widths[:, None]).reshape(-1)
    sizes = np.diff(offsets8.astype(np.int64))
    if np.any(sizes[~keep] != 0):
        raise ValueError("a slot behind an item's width holds a stream")
    return np.concatenate([offsets8[:-1][keep], offsets8[-1:]]).astype(np.uint64)


from .container import ContainerError, OpenTypedItems  # noqa: E402  (container.py reaches this module through its __getattr__ only)


class PackedTypedItems(OpenTypedItems):
    """What pack_typed_items_device leaves on the device: 8 streams an item in d_payload at d_offsets (slot q < width of item i is
    its plane q, stream 8 i + q; the others and those of items that were not split are empty), and beside them the pack call's own
    tables: d_kept (the item's length if it was split, else 0; its entry 8 i), d_widths, d_preds, d_count.  It is an OpenTypedItems
    that was never a file: decode_into is section 20's decode into staging and section 21's join, the lengths, widths and
    predictors looked up on the device, and to_bytes() makes the file."""

    def __init__(self, ctx, coder, d_kept, d_widths, d_preds, d_count, max_items, max_len, d_payload, d_offsets, d_stage, max_bytes):
        import torch
        from . import picks, typed_picks
        self.ctx, self._own, self.coder, self.nitems, self.max_len = ctx, False, coder, int(max_items), int(max_len)
        self.nsub, self.max_sub_len = SLOTS * self.nitems, int(max_len)
        self.crcs, self.d_stored = None, None
        self.d_kept, self._w8, self._p8, self.d_count = d_kept, d_widths, d_preds, d_count
        self.d_lengths = d_kept.view(-1, SLOTS)[:, 0] if self.nitems else torch.zeros(1, dtype=torch.int64, device="cuda")
        self.d_payload, self.d_offsets, self.payload_size = d_payload, d_offsets, d_payload.numel()
        self.d_sub_first = torch.arange(self.nitems + 1, dtype=torch.int64, device="cuda") * SLOTS
        self.max_bytes, self.d_stage = int(max_bytes), d_stage  # (the pack call's staging buffer: its split text is encoded by then)
        self._picks, self._join = picks, typed_picks

    def reserve(self, max_pick: int, max_bytes: int) -> None:
        """The scratch of decode_into calls with at most max_pick picks of at most max_bytes together: after it they allocate
        nothing in the context.  The staging buffer is the pack call's own, good for its max_bytes; a larger one is made here."""
        import torch
        self._picks.reserve(self.ctx, self.SLOTS * max_pick, self.max_sub_len, self.coder)
        self._join.reserve(self.ctx, self.SLOTS * max_pick, max_bytes)
        if max_bytes > self.max_bytes:
            self.max_bytes = int(max_bytes)
            self.d_stage = torch.zeros(max(self.max_bytes, 16), dtype=torch.uint8, device="cuda")

    def decode_into(self, d_pick, d_dst_at, d_count, d_dst, max_pick: int | None = None, stream=None) -> None:
        """OpenTypedItems.decode_into over the streams where the pack call left them: entry k < d_count[0]: item d_pick[k], decoded
        and joined -> d_dst[d_dst_at[k] : + its kept length].  Nothing is downloaded: an item that was not split has length 0 here,
        and its width and predictor are not looked at."""
        import torch
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            some = self.d_lengths[: max(self.nitems, 1)] > 0
            self.d_widths = torch.where(some, self._w8[: max(self.nitems, 1)].to(torch.int64), 1)
            self.d_preds = torch.where(some, self._p8[: max(self.nitems, 1)].to(torch.int64), 0)
        super().decode_into(d_pick, d_dst_at, d_count, d_dst, max_pick, stream)

    def verify(self, pick) -> None:
        raise ContainerError("a device-packed container has no checksums")

    def to_bytes(self) -> bytes:
        """Synchronises (a latched failure of either stage of the pack call is raised), downloads, drops the empty slots and writes
        the RCXJ version-1 container that pack_typed_items writes for the same items, widths and predictors, without checksums."""
        self.ctx.sync_status()
        from .layout import typed_items_header_bytes
        n = min(max(int(self.d_count[0]), 0), self.nitems)
        lengths = self.d_lengths[:n].cpu().numpy().astype(np.uint64)
        widths, preds = self._w8[:n].cpu().numpy(), self._p8[:n].cpu().numpy()
        offsets = compact_offsets(widths, self.d_offsets[: SLOTS * n + 1].cpu().numpy().astype(np.uint64))
        return typed_items_header_bytes(self.coder, lengths, widths, preds, offsets) + self.d_payload[: int(offsets[-1])].cpu().numpy().tobytes()


def pack_typed_items_device(ctx, d_src, d_src_at, d_len, d_widths, d_preds, d_count, max_items: int, max_len: int, max_bytes: int, coder: int = 0,
                            stream=None) -> PackedTypedItems:
    """Typed items that device code chose -- entry k < d_count[0] is d_src[d_src_at[k] : + d_len[k]] with width d_widths[k] and
    predictor d_preds[k] (int64 and uint8 cuda tensors [>= max_items], d_count one entry) -- split and encoded where they lie;
    reached as container.pack_typed_items_device.  Allocates the staging buffer, the payload and the tables once; after that it is
    torch ops and two calls on one stream (a chain under capture): the staging positions from the lengths, rcx_typed_split_picks_device
    into the staging buffer with d_kept, the expansion to 8 table slots an item, rcx_encode_picks_device over 8 * max_items entries.
    No download, no synchronisation -> PackedTypedItems.  No checksums.

    Both calls' tables have 8 entries an item (the split's: the item in its first slot), so a latched position of either stage is
    8 k + slot and PackedTypedItems.pick_of names the item.  An item is staged at the sum of the lengths in front of it, where a
    length above max_len (as a signed integer: also one with bit 63 set) or at or behind the count counts as 0, so one garbage
    length does not move the others.  Such an item above max_len is given a destination past the staging buffer and is latched by
    the split: RCX_E_CAPACITY at its pick -- RCX_E_CORRUPT where its width or predictor is bad too or its length above what one
    superblock takes (rcx_tpick_validate looks at those first).  reserve: typed_split_picks.reserve(ctx, 8 * max_items, max_bytes)
    and encode_picks.reserve(ctx, 8 * max_items, max_len, max_bytes, coder) make the two calls launches only."""
    import torch
    from . import encode_picks
    S = SLOTS
    _table(d_src, 0, "d_src", 1)  # (host tensors are refused before anything is allocated)
    for t, least, what, size in ((d_src_at, max_items, "d_src_at", 8), (d_len, max_items, "d_len", 8), (d_widths, max_items, "d_widths", 1),
                                 (d_preds, max_items, "d_preds", 1), (d_count, 1, "d_count", 8)):
        _table(t, least, what, size)
    stage_cap = max(int(max_bytes), 16)
    d_stage = torch.zeros(stage_cap, dtype=torch.uint8, device="cuda")
    d_payload = torch.empty(max(encode_picks.dst_bound(S * max_items, max_bytes, coder), 16), dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(S * max_items + 1, dtype=torch.int64, device="cuda")
    d_kept = torch.zeros(max(S * max_items, 1), dtype=torch.int64, device="cuda")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        n = d_len[:max_items]
        meant = torch.arange(max_items, device=n.device) < d_count[:1]
        fits = meant & (n >= 0) & (n <= max_len)
        zero = torch.zeros_like(n)
        counted = torch.where(fits, n, zero)
        stage_at = torch.cumsum(counted, 0) - counted
        q = torch.arange(S, device=n.device).unsqueeze(0)
        first = (q == 0).to(torch.int64)
        # the split's tables: the item in its first slot; one that does not fit goes past the staging buffer, which latches it
        src_at = (torch.where(meant, d_src_at[:max_items], zero).unsqueeze(1) * first).contiguous().view(-1)
        dst_at = (torch.where(fits, stage_at, torch.full_like(n, stage_cap + 1)).unsqueeze(1) * first).contiguous().view(-1)
        length = (torch.where(meant, n, zero).unsqueeze(1) * first).contiguous().view(-1)
        widths = (torch.where(meant, d_widths[:max_items].to(torch.int64), torch.ones_like(n)).unsqueeze(1) * first + (1 - first)).to(torch.uint8).contiguous().view(-1)
        preds = (torch.where(meant, d_preds[:max_items].to(torch.int64), zero).unsqueeze(1) * first).to(torch.uint8).contiguous().view(-1)
        count = torch.clamp(d_count[:1], 0, max_items) * S
    if max_items:
        split_device(ctx, d_src, src_at, dst_at, length, widths, preds, count, d_stage, int(max_bytes), max_pick=S * max_items, kept=d_kept, stream=stream,
                     dst_cap=stage_cap)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        # the encode call's tables from kept: slot q < w is plane q, m bytes at q * m of the item's staging span, the last with the tail
        kept = d_kept[: S * max_items].view(-1, S)[:, 0]
        w = torch.where(kept > 0, d_widths[:max_items].to(torch.int64), torch.ones_like(kept))
        m = (kept // w).unsqueeze(1)
        tail = (kept - (kept // w) * w).unsqueeze(1)
        live = q < w.unsqueeze(1)
        sub_len = torch.where(live, m + torch.where(q == w.unsqueeze(1) - 1, tail, torch.zeros_like(tail)), torch.zeros_like(q)).contiguous().view(-1)
        sub_at = (stage_at.unsqueeze(1) + q * m).contiguous().view(-1)
    if max_items:
        encode_picks.encode_device(ctx, d_stage, sub_at, sub_len, count, d_payload, d_offsets, int(max_len), int(max_bytes), max_items=S * max_items, coder=coder,
                                   stream=stream, src_cap=stage_cap)
    packed = PackedTypedItems(ctx, coder, d_kept, d_widths, d_preds, d_count, max_items, max_len, d_payload, d_offsets, d_stage, max_bytes)
    packed.stage_at = stage_at  # int64[max_items]: where each item's split text was staged (garbage lengths do not move it)
    return packed
