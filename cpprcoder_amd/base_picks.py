"""ctypes binding of include/rcx_base_picks.h: the join per item of base_items.py whose tables -- where each item's split text
lies, where its base span lies, where its joined bytes go, its length, width, predictor and op, how many entries are meant --
lie in device memory.  The call plans on the GPU and only enqueues, so it can follow picks.decode_device inside one captured
graph.

    entry k < min(count, max_pick):   join of src[src_at[k] : + len[k]]  ->  dst[dst_at[k] : + len[k]],
                                      with an op against base[base_at[k] : + len[k]]

What is checked moves to the device with the tables: a bad entry is skipped and latched, every other entry joins, and when the
valid entries have more than max_bytes between them nothing is joined (include/rcx_base_picks.h has the contract in full).
plan_numpy is the planner's rules in numpy, down to both sets' tables; it is the mirror the tests hold the kernels to.  The
calls themselves are host plumbing like rcx.py: every device table is a torch cuda tensor, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .base_items import NO_BASE
from .base import SUBZZ
from .predict import ZIGZAG
from .typed_picks import (BINS, HEAD_BYTES, MAX_BLOCK, MAX_BYTES, MAX_PICK, PLAN_THREADS, ROW, ROW_BYTES, TYPED_STEP_ROWS, _table, bin_of,  # noqa: F401
                          set_tables as _set_tables)  # (the planner's constants and its rendering of a set are shared)

# every symbol include/rcx_base_picks.h declares
EXPORTS = ("rcx_base_picks_reserve", "rcx_base_picks_scratch_bytes", "rcx_base_join_picks_device", "rcx_base_join_picks")

NONE, ROWS, SCAN, BASE = 0, 1, 2, 3  # an entry's route: not joined; the typed set's classes; its scan list; the base set
BASE_STEP_ROWS = {1: 8, 2: 4, 4: 2, 8: 1}    # RCX_BASE_ROWS(w): ... of the base set

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_base_picks.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_base_picks_reserve.restype, L.rcx_base_picks_reserve.argtypes = i32, [vp, u64, u64]
        L.rcx_base_picks_scratch_bytes.restype, L.rcx_base_picks_scratch_bytes.argtypes = u64, [u64, u64]
        L.rcx_base_join_picks_device.restype = i32  # ctx, src, cap, base, cap, src_at, base_at, dst_at, len, widths, preds, ops, count, max_pick, max_bytes, dst, cap, stream
        L.rcx_base_join_picks_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, u64, u64, vp, u64, vp]
        L.rcx_base_join_picks.restype = i32  # ctx, src, cap, base, cap, src_at, base_at, dst_at, len, widths, preds, ops, npick, dst, cap
        L.rcx_base_join_picks.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp, u64]
        _ready = True
    return L


# ---- the planner's rules, in numpy -----------------------------------------------------------------------------------------
def scratch_formula(max_pick: int, max_bytes: int) -> int:
    """The formula of include/rcx_base_picks.h for rcx_base_picks_scratch_bytes."""
    if not (0 < max_pick <= MAX_PICK and 0 <= max_bytes <= MAX_BYTES):
        return 0
    tiles = (max_pick + PLAN_THREADS - 1) // PLAN_THREADS
    rows, base_rows = max_bytes // ROW_BYTES + 8, max_bytes // ROW_BYTES + 24
    n = (2 * HEAD_BYTES + 16 * (max_pick + 1) + 56 * max_pick + 264 * tiles + 64 * tiles + 16 * max_pick + 4 * (rows + base_rows) + 8 * BINS + 8
         + max_pick)
    return (n + 7) // 8 * 8


def _class_of(w: int, second: int) -> int:
    return 3 * (1, 2, 4, 8).index(w) + second


def plan_numpy(src_at, base_at, dst_at, length, widths, preds, ops, count: int, max_bytes: int, src_cap: int, base_cap: int, dst_cap: int):
    """What the planner of rcx_base_join_picks_device decides for these tables (max_pick = len(length)) -> dict:
        count     min(count, max_pick), how many entries are read
        valid     bool[max_pick]: the entry passed the checks (it is joined unless the call overflows)
        route     uint8[max_pick]: NONE (not meant, empty, skipped, or the call overflowed), ROWS, SCAN or BASE
        bins      int64[max_pick]: a SCAN entry's bin in work order, else -1 (the order inside a bin is not the model's)
        bytes     what the valid entries have between them
        overflow  bytes > max_bytes: nothing is joined
        status    what rcx_ctx_sync_status returns: OK, E_CORRUPT or E_CAPACITY
        position  the lowest failing position, None without a failure
        typed     the typed set's tables (the head's five arrays, ufirst, entry = the call's entry at each place, rowtab):
                  the entries without an op and without a predictor, in 4 of 12 classes
        base      the base set's, class 3 * log2(width) + op, and bat = the base offset at each place
    Entries at or past the count are not read: they may hold anything.  preds, ops and base_at may be None."""
    src_at, dst_at, length = (np.asarray(x, dtype=np.uint64) for x in (src_at, dst_at, length))
    widths = np.asarray(widths, dtype=np.uint8)
    max_pick = len(length)
    preds = np.zeros(max_pick, np.uint8) if preds is None else np.asarray(preds, dtype=np.uint8)
    ops = np.full(max_pick, NO_BASE, np.uint8) if ops is None else np.asarray(ops, dtype=np.uint8)
    base_at = np.zeros(max_pick, np.uint64) if base_at is None else np.asarray(base_at, dtype=np.uint64)
    if not (len(src_at) == len(dst_at) == len(base_at) == len(widths) == len(preds) == len(ops) == max_pick):
        raise ValueError("one source, base, destination, length, width, predictor and op per entry")
    meant = min(int(count), max_pick)
    valid = np.zeros(max_pick, dtype=bool)
    route = np.zeros(max_pick, dtype=np.uint8)
    bins = np.full(max_pick, -1, dtype=np.int64)
    corrupt, capacity = [], []
    if int(count) > max_pick:
        capacity.append(max_pick)
    total = 0
    placed = ([], [])
    for k in range(meant):
        n, w, p, o, a, b = int(length[k]), int(widths[k]), int(preds[k]), int(ops[k]), int(src_at[k]), int(dst_at[k])
        if n == 0:
            continue
        if (w not in (1, 2, 4, 8) or p > ZIGZAG or (w == 1 and p) or (o != NO_BASE and (o > SUBZZ or p)) or n // w + n % w > MAX_BLOCK):
            corrupt.append(k)
        elif a + n > src_cap or b + n > dst_cap or (o != NO_BASE and int(base_at[k]) + n > base_cap):  # (Python's integers: no sum wraps)
            capacity.append(k)
        else:
            valid[k] = True
            total += n
            if o != NO_BASE:
                route[k] = BASE
                placed[1].append((_class_of(w, o), k, n, w))
            elif p:
                route[k], bins[k] = SCAN, bin_of(n)
            else:
                route[k] = ROWS
                placed[0].append((_class_of(w, 0), k, n, w))
    overflow = total > max_bytes
    if overflow:
        capacity.append(meant)
        route[:] = NONE
        placed = ([], [])
    failing = corrupt + capacity
    typed, based = _set_tables(placed[0], TYPED_STEP_ROWS), _set_tables(placed[1], BASE_STEP_ROWS)
    based["bat"] = base_at[based["entry"]]
    return {"count": meant, "valid": valid, "route": route, "bins": bins, "bytes": total, "overflow": overflow,
            "status": rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if capacity else rcx.OK, "position": min(failing) if failing else None,
            "typed": typed, "base": based}


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(max_pick: int, max_bytes: int) -> int:
    """rcx_base_picks_scratch_bytes: what Context.scratch_bytes() reports for a fresh context after reserve(); 0 for bad arguments."""
    if not (0 <= max_pick < 1 << 64 and 0 <= max_bytes < 1 << 64):
        return 0
    return int(lib().rcx_base_picks_scratch_bytes(max_pick, max_bytes))


def reserve(ctx, max_pick: int, max_bytes: int) -> None:
    """rcx_base_picks_reserve: after it, join_device with at most max_pick entries of at most max_bytes together allocates nothing."""
    rcx._check(lib().rcx_base_picks_reserve(ctx._h, max_pick, max_bytes), "rcx_base_picks_reserve")


def join_device(ctx, src, base, src_at, base_at, dst_at, length, widths, preds, ops, count, dst, max_bytes: int, max_pick: int | None = None, stream=None,
                src_cap: int | None = None, base_cap: int | None = None, dst_cap: int | None = None) -> None:
    """src, base, dst: uint8 cuda tensors, dst apart from both; src_at, base_at, dst_at, length: int64 cuda tensors [>= max_pick]
    (max_pick = length.numel() if None); widths, preds, ops: uint8 cuda tensors [>= max_pick]; preds may be None, ops may be None
    and then base and base_at too; count: int64 cuda tensor of one entry.  Enqueues only; after reserve() it may be captured in
    a graph."""
    max_pick = length.numel() if max_pick is None else int(max_pick)
    if not 0 <= max_pick <= MAX_PICK:
        raise ValueError("max_pick is 0 .. 2^31 - 1")
    if not 0 <= max_bytes <= MAX_BYTES:
        raise ValueError("max_bytes is 0 .. 2^42")
    src_cap = src.numel() if src_cap is None else int(src_cap)
    dst_cap = dst.numel() if dst_cap is None else int(dst_cap)
    base_cap = (0 if base is None else base.numel()) if base_cap is None else int(base_cap)
    args = (_table(src, src_cap, "src", 1), src_cap, None if base is None else _table(base, base_cap, "base", 1), base_cap,
            _table(src_at, max_pick, "src_at", 8), None if base_at is None else _table(base_at, max_pick, "base_at", 8),
            _table(dst_at, max_pick, "dst_at", 8), _table(length, max_pick, "length", 8), _table(widths, max_pick, "widths", 1),
            None if preds is None else _table(preds, max_pick, "preds", 1), None if ops is None else _table(ops, max_pick, "ops", 1),
            _table(count, 1, "count", 8), max_pick, max_bytes, _table(dst, dst_cap, "dst", 1), dst_cap)
    rcx._check(lib().rcx_base_join_picks_device(ctx._h, *args, ctx._stream_handle(stream)), "rcx_base_join_picks_device")


def join(ctx, src, base, src_at, base_at, dst_at, length, widths, preds, ops, dst: np.ndarray):
    """rcx_base_join_picks on host buffers: every entry is meant; dst (uint8, written in place) -> the latched status (OK,
    E_CORRUPT or E_CAPACITY).  The good entries are written also behind a latched failure."""
    x = rcx._np_u8(src)
    ref = None if base is None else np.ascontiguousarray(rcx._np_u8(base))
    a, b, n = (np.ascontiguousarray(t, dtype=np.uint64) for t in (src_at, dst_at, length))
    at = None if base_at is None else np.ascontiguousarray(base_at, dtype=np.uint64)
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    p = None if preds is None else np.ascontiguousarray(preds, dtype=np.uint8)
    o = None if ops is None else np.ascontiguousarray(ops, dtype=np.uint8)
    if not (len(a) == len(b) == len(w) == len(n)) or any(t is not None and len(t) != len(n) for t in (p, o, at)):
        raise ValueError("one source, base, destination, length, width, predictor and op per entry")
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
        raise ValueError("dst is a writable contiguous uint8 array")
    ptr = lambda t: None if t is None or not len(t) else t.ctypes.data  # noqa: E731
    st = lib().rcx_base_join_picks(ctx._h, x.ctypes.data, len(x), ptr(ref), 0 if ref is None else len(ref), a.ctypes.data, ptr(at), b.ctypes.data,
                                   n.ctypes.data, w.ctypes.data, ptr(p), ptr(o), len(n), dst.ctypes.data, len(dst))
    if st in (rcx.E_ARG, rcx.E_HIP, rcx.E_NOMEM):
        raise rcx.RcxError(st, "rcx_base_join_picks")
    return st
