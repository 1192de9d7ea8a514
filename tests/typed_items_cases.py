"""What the typed item tests share (tests/test_typed_items_cpu.py, tests/test_gpu_typed_items.py): batches of typed items
around every switch point of the kernels (csrc/rcx_typed_items.hpp), their bytes, and the expectation composed from
planes_cases / predict_cases -- an item is one superblock of those.  Not a test file."""
import numpy as np

import planes_cases as pc
import predict_cases as pr

WIDTHS = (1, 2, 4, 8)
NONE, DELTA, ZIGZAG = pr.NONE, pr.DELTA, pr.ZIGZAG
OFFSETS = pc.OFFSETS
KINDS = pr.KINDS  # random, minus_k, ramp (the width-8 items of a batch)
PLANES_U4 = 16    # RCX_PLANES_U4: a workgroup step is PLANES_U4 / w rows of 256 units


def preds_of(width):
    return (NONE,) if width == 1 else (NONE, DELTA, ZIGZAG)


def switch_lengths(w):
    """Item lengths in bytes around every switch point for width w: nothing, below and at one element, around one unit and
    17 of them, 64 units (a wave, and the scan's tile of 1024 elements) +- one element, 256 units (a row) +- one, one workgroup
    step +- one element, 2 tiles + 5 elements; and each of the larger ones again with a ragged tail."""
    step = PLANES_U4 // w * 256 * 16 if w > 1 else 16 * 256 * 16  # elements of a workgroup step
    elements = [1024 - 1, 1024, 1024 + 1, 4096 - 1, 4096, 4096 + 1, step - 1, step, step + 1, 2 * 1024 + 5]
    out = [0, 1, w - 1, w, 16 * w - 1, 16 * w, 16 * w + 1, 17 * 16 * w]
    out += [e * w for e in elements]
    out += [e * w + (k % w) for k, e in enumerate(elements, 1) if w > 1]
    return [n for n in out if n >= 0]


def _case(name, items, k):
    lens, widths, preds = (np.array([it[j] for it in items], dtype) for j, dtype in ((0, np.uint64), (1, np.uint8), (2, np.uint8)))
    return {"name": name, "lengths": lens, "widths": widths, "preds": preds, "src_offset": OFFSETS[k % 5], "dst_offset": OFFSETS[(k // 5 + k) % 5]}


def kernel_cases():
    """A list of batches: dict(name, lengths, widths, preds, src_offset, dst_offset).  The offsets cycle through all 25 pairs."""
    out = []
    # one class a batch: every switch length, so that rows, steps and scan tiles begin and end inside and between items
    for w in WIDTHS:
        for p in preds_of(w):
            out.append(_case(f"switch w={w} p={p}", [(n, w, p) for n in switch_lengths(w)], len(out)))
    # neighbours of different width and predictor inside one wave's and one workgroup's turn: small items, classes in turn
    classes = [(w, p) for w in WIDTHS for p in preds_of(w)]
    rs = np.random.RandomState(5)
    small = [(int(rs.randint(0, 6 * 16 * w + w)), w, p) for k in range(700) for (w, p) in [classes[k % len(classes)]]]
    out.append(_case("mixed small", small, len(out)))
    # many items to a row and more than one step in every class: 1 to 64 / w units each, with rests and tails
    out.append(_case("mixed many", [(int(rs.randint(16 * w, 1024 + w)), w, p) for k in range(6000) for (w, p) in [classes[(k * 7) % len(classes)]]],
                     len(out)))
    # runs of empty items: in front, between, behind, and a batch of nothing else
    run = [(0, 4, DELTA)] * 70
    out.append(_case("empty runs", run + [(100, 2, ZIGZAG)] + run + [(0, 1, NONE)] * 3 + [(4099, 8, DELTA), (33, 1, NONE)] + run, len(out)))
    out.append(_case("only empty", run, len(out)))
    out.append(_case("no items", [], len(out)))
    # large and small side by side: a row that begins in a large item and ends in small ones, and the other way
    out.append(_case("large and small", [(5, 2, NONE), (2 * 4099, 2, NONE), (64, 2, NONE), (7, 2, NONE), (2 * 300, 2, NONE), (2 * 5000, 2, NONE), (31, 2, NONE)]
                     + [(4 * 16 * 255, 4, ZIGZAG), (4 * 16, 4, ZIGZAG), (4 * 16 * 3 + 3, 4, ZIGZAG)] + [(8 * 16 * 511, 8, DELTA), (8 * 16 * 2, 8, DELTA)], len(out)))
    for k in range(len(out), 25):  # (so that every pair of offsets occurs)
        out.append(_case(f"offsets {k}", [(int(rs.randint(0, 3000)), w, p) for (w, p) in classes], k))
    return out


def offsets_of(case, base=0):
    offs = np.zeros(len(case["lengths"]) + 1, np.uint64)
    np.cumsum(case["lengths"], out=offs[1:])
    return offs + np.uint64(base)


def case_bytes(case, kind, noise):
    """The batch's bytes: `random` from noise; `minus_k`: every item of width above 1 holds the elements -k (every difference
    all 0xFF); `ramp`: the width-8 items hold 2^32 - 8 + k, the others noise."""
    total = int(case["lengths"].sum())
    x = noise[:total].copy()
    if kind == "random":
        return x
    at = 0
    for n, w in zip(case["lengths"].astype(np.int64), case["widths"]):
        if kind == "minus_k" and w > 1:
            x[at: at + n] = pr.kernel_data("minus_k", int(w), int(n), None)
        elif kind == "ramp" and w == 8:
            x[at: at + n] = pr.kernel_data("ramp", 8, int(n), None)
        at += int(n)
    return x


def _each(case, x, fn):
    out, at = x.copy(), 0
    for n, w, p in zip(case["lengths"].astype(np.int64), case["widths"], case["preds"]):
        n, w, p = int(n), int(w), int(p)
        if w > 1 and n >= w:  # one superblock: a block of m + 1 elements holds the m elements and the tail
            out[at: at + n] = fn(x[at: at + n], w, n // w + 1, p)
        at += n
    return out


def split_expected(case, x):
    """Item by item what rcx_predict_split makes of it as one superblock (tests/predict_cases.py)."""
    return _each(case, x, pr.split_numpy)


def join_expected(case, y):
    return _each(case, y, pr.join_numpy)


def superblock_items(n, width, block, pred):
    """A buffer of n bytes cut into items of width * block bytes, its ragged rest as the last -> (lengths, widths, preds)."""
    sb = width * block
    lengths = [sb] * (n // sb) + ([n % sb] if n % sb else [])
    return np.array(lengths, np.uint64), np.full(len(lengths), width, np.uint8), np.full(len(lengths), pred, np.uint8)


def write_cases(path, cases):
    """The batches as the text tests/sim/typed_items_san.cpp reads: per batch `nitems base`, then a line `len width pred` per item."""
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for k, c in enumerate(cases):
            f.write(f"{len(c['lengths'])} {(k * 37) % 101}\n")
            for n, w, p in zip(c["lengths"], c["widths"], c["preds"]):
                f.write(f"{int(n)} {int(w)} {int(p)}\n")
