"""ctypes binding of include/rcx_typed_picks.h: the typed join per item whose tables -- where each item's split text lies, where
its joined bytes go, its length, width and predictor, how many entries are meant -- lie in device memory.  The call plans on
the GPU and only enqueues, so it can follow picks.decode_device inside one captured graph.

    entry k < min(count, max_pick):   join of src[src_at[k] : + len[k]]  ->  dst[dst_at[k] : + len[k]]

What is checked moves to the device with the tables: a bad entry is skipped and latched, every other entry joins, and when the
valid entries have more than max_bytes between them nothing is joined (include/rcx_typed_picks.h has the contract in full).
plan_numpy is those rules in numpy and bin_of the scan list's work order; they are the mirror the tests hold the kernels to.
The calls themselves are host plumbing like rcx.py: every device table is a torch cuda tensor, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import rcx
from .picks import len_bin
from .predict import ZIGZAG

# every symbol include/rcx_typed_picks.h declares
EXPORTS = ("rcx_typed_picks_reserve", "rcx_typed_picks_scratch_bytes", "rcx_typed_join_picks_device", "rcx_typed_join_picks")

MAX_PICK = 0x7FFFFFFF
MAX_BYTES = 1 << 42          # RCX_TPICK_MAX_BYTES: the row table has 32-bit indices
MAX_BLOCK = (1 << 24) - 256  # RCX_MAX_BLOCK: len // w + len % w of an entry at the most
PLAN_THREADS = 256           # RCX_TPICK_THREADS: entries of a tile = what a workgroup of the planner takes at a go
PLAN_GRID = 512              # RCX_TPICK_GRID: workgroups of the planner's entry kernels at the most; behind it they go round
PLAN_TOP = 1024              # RCX_TPICK_TOP: tiles a pass of the one workgroup that sums over the tiles
SCAN_TILE = 1024             # elements of the scan kernel's tile (RCX_PREDICT_TILE_UNITS units of 16)
EXACT = 512                  # RCX_TPICK_EXACT: scan list lengths below this have a bin each
BINS = EXACT + (27 - 9) * 256  # RCX_TPICK_BINS
ROW_BYTES = 4096             # bytes of a row of 256 units at the least
HEAD_BYTES = 400             # sizeof(RcxTypedClasses)
ROW = 256                    # RCX_TYPED_ROW: units of a row
TYPED_STEP_ROWS = {1: 16, 2: 8, 4: 4, 8: 2}  # RCX_PLANES_U4 / w: rows of a workgroup step of the typed kernels
NONE, ROWS, SCAN = 0, 1, 2   # an entry's route: not joined; the classes without a predictor; the scan list

_ready = False


def lib() -> C.CDLL:
    """rcx.lib() with the signatures of the four calls of include/rcx_typed_picks.h set."""
    global _ready
    L = rcx.lib()
    if not _ready:
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        L.rcx_typed_picks_reserve.restype, L.rcx_typed_picks_reserve.argtypes = i32, [vp, u64, u64]
        L.rcx_typed_picks_scratch_bytes.restype, L.rcx_typed_picks_scratch_bytes.argtypes = u64, [u64, u64]
        L.rcx_typed_join_picks_device.restype = i32
        L.rcx_typed_join_picks_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u64, vp, u64, vp]
        L.rcx_typed_join_picks.restype = i32
        L.rcx_typed_join_picks.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, u64]
        _ready = True
    return L


# ---- the planner's rules, in numpy -----------------------------------------------------------------------------------------
def bin_of(length: int) -> int:
    """The bin of a scan list entry of `length` bytes, 1 <= length < 2^27: picks.len_bin among BINS."""
    return len_bin(length, 27)


def head_of(nent, units, step_rows):
    """rcx_class_head: the head of a set from its 12 classes' entries and whole units; step_rows[w] = the rows of a workgroup
    step of width w -> (ent_first[13], row_first[13], ubase[13], step_end[12], rest_end[12]) of Python integers."""
    ent_first, row_first, ubase, step_end, rest_end = [], [], [], [], []
    ents = rows = ub = steps = rests = 0
    for c in range(12):
        w = 1 << (c // 3)
        n, un = int(nent[c]), int(units[c])
        ent_first.append(ents), row_first.append(rows), ubase.append(ub)
        step = step_rows[w] * ROW
        steps += -(-un // step)
        rests += -(-n * 17 * w // ROW)
        step_end.append(steps), rest_end.append(rests)
        ents, ub = ents + n, ub + un
        if n:
            rows += -(-un // ROW) + 1
    return ent_first + [ents], row_first + [rows], ubase + [ub], step_end, rest_end


def set_tables(placed, step_rows):
    """One set's tables from its entries [(class, k, len, width)] in the caller's order -> dict(ent_first, row_first, ubase,
    step_end, rest_end: the head; ufirst; entry: which entry of the call stands at each place; rowtab)."""
    nent, units = [0] * 12, [0] * 12
    for c, _, n, w in placed:
        nent[c] += 1
        units[c] += (n // w) >> 4
    ent_first, row_first, ubase, step_end, rest_end = head_of(nent, units, step_rows)
    ents, rows = ent_first[12], row_first[12]
    ufirst, entry = np.zeros(ents + 1, np.uint64), np.zeros(ents, np.int64)
    nxt, unit = list(ent_first[:12]), list(ubase[:12])
    for c, k, n, w in placed:
        ufirst[nxt[c]], entry[nxt[c]] = unit[c], k
        nxt[c] += 1
        unit[c] += (n // w) >> 4
    ufirst[ents] = ubase[12]
    rowtab = np.zeros(rows, np.uint32)
    for c in range(12):
        if not nent[c]:
            continue
        last, k = ent_first[c + 1] - 1, ent_first[c]
        nrow = -(-units[c] // ROW)
        for r in range(nrow):
            g = ubase[c] + r * ROW
            while k < last and int(ufirst[k + 1]) <= g:
                k += 1
            rowtab[row_first[c] + r] = k
        rowtab[row_first[c] + nrow] = last
    return {"ent_first": np.array(ent_first, np.uint32), "row_first": np.array(row_first, np.uint32), "ubase": np.array(ubase, np.uint64),
            "step_end": np.array(step_end, np.uint64), "rest_end": np.array(rest_end, np.uint64), "ufirst": ufirst, "entry": entry, "rowtab": rowtab}


def scratch_formula(max_pick: int, max_bytes: int) -> int:
    """The formula of include/rcx_typed_picks.h for rcx_typed_picks_scratch_bytes."""
    if not (0 < max_pick <= MAX_PICK and 0 <= max_bytes <= MAX_BYTES):
        return 0
    tiles, rows = (max_pick + PLAN_THREADS - 1) // PLAN_THREADS, max_bytes // ROW_BYTES + 8
    n = HEAD_BYTES + 8 * (max_pick + 1) + 32 * max_pick + 72 * tiles + 16 * tiles + 12 * max_pick + 4 * rows + 8 * BINS + 8 + max_pick
    return (n + 7) // 8 * 8


def plan_numpy(src_at, dst_at, length, widths, preds, count: int, max_bytes: int, src_cap: int, dst_cap: int):
    """What the planner of rcx_typed_join_picks_device decides for these tables (max_pick = len(length)) -> dict:
        count     min(count, max_pick), how many entries are read
        valid     bool[max_pick]: the entry passed the checks (it is joined unless the call overflows)
        route     uint8[max_pick]: NONE (not meant, empty, skipped, or the call overflowed), ROWS or SCAN
        bins      int64[max_pick]: a SCAN entry's bin in work order, else -1
        bytes     what the valid entries have between them
        overflow  bytes > max_bytes: nothing is joined
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
    route = np.zeros(max_pick, dtype=np.uint8)
    bins = np.full(max_pick, -1, dtype=np.int64)
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
            valid[k] = True
            total += n
            route[k] = SCAN if p else ROWS
            if p:
                bins[k] = bin_of(n)
    overflow = total > max_bytes
    if overflow:
        capacity.append(meant)
        route[:] = NONE
    failing = corrupt + capacity
    return {"count": meant, "valid": valid, "route": route, "bins": bins, "bytes": total, "overflow": overflow,
            "status": rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if capacity else rcx.OK, "position": min(failing) if failing else None}


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def scratch_bytes(max_pick: int, max_bytes: int) -> int:
    """rcx_typed_picks_scratch_bytes: what Context.scratch_bytes() reports for a fresh context after reserve(); 0 for bad arguments."""
    if not (0 <= max_pick < 1 << 64 and 0 <= max_bytes < 1 << 64):
        return 0
    return int(lib().rcx_typed_picks_scratch_bytes(max_pick, max_bytes))


def reserve(ctx, max_pick: int, max_bytes: int) -> None:
    """rcx_typed_picks_reserve: after it, join_device with at most max_pick entries of at most max_bytes together allocates nothing."""
    rcx._check(lib().rcx_typed_picks_reserve(ctx._h, max_pick, max_bytes), "rcx_typed_picks_reserve")


def _table(t, least: int, what: str, size: int):
    """A device table of `size`-byte integers with `least` entries at least."""
    if not getattr(t, "is_cuda", False):
        raise ValueError(f"{what} is a torch cuda tensor: the call reads it on the device")
    if t.element_size() != size or t.is_floating_point() or not t.is_contiguous():
        raise ValueError(f"{what} holds contiguous {8 * size}-bit integers")
    if t.numel() < least:
        raise ValueError(f"{what} needs {least} entries")
    return t.data_ptr()


def join_device(ctx, src, src_at, dst_at, length, widths, preds, count, dst, max_bytes: int, max_pick: int | None = None, stream=None,
                src_cap: int | None = None, dst_cap: int | None = None) -> None:
    """src, dst: uint8 cuda tensors that do not overlap; src_at, dst_at, length: int64 cuda tensors [>= max_pick] (max_pick =
    length.numel() if None); widths, preds: uint8 cuda tensors [>= max_pick], preds may be None; count: int64 cuda tensor of one
    entry.  Enqueues only; after reserve() it may be captured in a graph."""
    max_pick = length.numel() if max_pick is None else int(max_pick)
    if not 0 <= max_pick <= MAX_PICK:
        raise ValueError("max_pick is 0 .. 2^31 - 1")
    if not 0 <= max_bytes <= MAX_BYTES:
        raise ValueError("max_bytes is 0 .. 2^42")
    src_cap = src.numel() if src_cap is None else int(src_cap)
    dst_cap = dst.numel() if dst_cap is None else int(dst_cap)
    args = (_table(src, src_cap, "src", 1), src_cap, _table(src_at, max_pick, "src_at", 8), _table(dst_at, max_pick, "dst_at", 8),
            _table(length, max_pick, "length", 8), _table(widths, max_pick, "widths", 1), None if preds is None else _table(preds, max_pick, "preds", 1),
            _table(count, 1, "count", 8), max_pick, max_bytes, _table(dst, dst_cap, "dst", 1), dst_cap)
    rcx._check(lib().rcx_typed_join_picks_device(ctx._h, *args, ctx._stream_handle(stream)), "rcx_typed_join_picks_device")


def join(ctx, src, src_at, dst_at, length, widths, preds, dst: np.ndarray):
    """rcx_typed_join_picks on host buffers: every entry is meant; dst (uint8, written in place) -> the latched status (OK,
    E_CORRUPT or E_CAPACITY).  The good entries are written also behind a latched failure."""
    x = rcx._np_u8(src)
    a, b, n = (np.ascontiguousarray(t, dtype=np.uint64) for t in (src_at, dst_at, length))
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    p = None if preds is None else np.ascontiguousarray(preds, dtype=np.uint8)
    if not (len(a) == len(b) == len(w) == len(n)) or (p is not None and len(p) != len(n)):
        raise ValueError("one source, destination, length, width and predictor per entry")
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
        raise ValueError("dst is a writable contiguous uint8 array")
    st = lib().rcx_typed_join_picks(ctx._h, x.ctypes.data, len(x), a.ctypes.data, b.ctypes.data, n.ctypes.data, w.ctypes.data,
                                    None if p is None else p.ctypes.data, len(n), dst.ctypes.data, len(dst))
    if st in (rcx.E_ARG, rcx.E_HIP, rcx.E_NOMEM):
        raise rcx.RcxError(st, "rcx_typed_join_picks")
    return st
