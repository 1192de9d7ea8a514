"""The batches, data and tables of the candidate-cost tests (include/rcx_typed_stats.h): tests/test_typed_stats_cpu.py and
tests/test_gpu_typed_stats.py build them here.  Plain numpy, no GPU."""
import numpy as np

import base_items_cases as bc
from cpprcoder_amd import typed_stats as ts

WIDTHS = (1, 2, 4, 8)
OFFSETS = (0, 1, 3, 8, 15)
LAYOUTS = bc.LAYOUTS  # where the base spans lie: in item order, in reverse order, all at offset 0
KINDS = bc.KINDS + ("constant", "alternating")
UNIT = 16          # elements a lane takes at a time (csrc/rcx_typed_stats.hpp)
WAVE_PASS = 64     # units a wave takes at a time
GROUP_PASS = 256   # units a workgroup takes at a time: one row in flight


def masks_of(width):
    """Each bit alone, the predictors, the ops, everything a width may ask for, and nothing."""
    if width == 1:
        return [1, 8, 16, 32, ts.OP_BITS, ts.ALL_OPS, 0]
    return [1, 2, 4, 8, 16, 32, ts.ALL_PREDS, ts.OP_BITS, ts.ALL_OPS, ts.ALL, 0]


def switch_lengths(w):
    """Item lengths in bytes at which rcx_typed_stats_k<w> changes what it does: nothing, less than an element, 15 to 17
    elements around the unit, one element either side of a wave's pass and of a workgroup's pass (and of two), w * 65536 and
    the same with w - 1 tail bytes."""
    out = [0, 1, w - 1, w, w + 1]
    for elements in (UNIT, UNIT * WAVE_PASS, UNIT * GROUP_PASS, 2 * UNIT * GROUP_PASS):
        out += [(elements - 1) * w, elements * w, (elements + 1) * w + (w - 1)]
    out += [w * 65536, w * 65536 + w - 1]
    return sorted(set(n for n in out if n >= 0))


def offsets_of(lengths, first=0):
    offs = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(np.asarray(lengths, np.uint64), out=offs[1:])
    return offs + np.uint64(first)


def layout_of(lengths, masks, layout, first=0):
    """-> (base_offsets uint64[nitems], bytes of the base behind `first`): bc.base_layout for the items whose mask has an op bit;
    the others get an offset far outside, which nobody may look at."""
    case = {"lengths": np.asarray(lengths, np.uint64), "ops": np.where(np.asarray(masks) & ts.OP_BITS, 2, bc.NO_BASE).astype(np.uint8), "layout": layout}
    return bc.base_layout(case, first)


def data_of(lengths, widths, masks, layout, kind, noise):
    """-> (source, base).  bc.case_data's four kinds for the items that ask for an op; constant: every element of the source is
    one value; alternating: two values in turn -- the skew the none and delta planes see."""
    lengths, widths, masks = np.asarray(lengths, np.uint64), np.asarray(widths, np.uint8), np.asarray(masks, np.uint8)
    case = {"lengths": lengths, "widths": widths, "ops": np.where(masks & ts.OP_BITS, 2, bc.NO_BASE).astype(np.uint8), "layout": layout}
    x, ref = bc.case_data(case, kind if kind in bc.KINDS else "random", noise)
    if kind in bc.KINDS:
        return x, ref
    at = 0
    for n, w in zip(lengths.astype(np.int64), widths):
        n, w = int(n), int(w)
        m = n // w
        if m:
            two = x[at: at + 2 * w].copy() if m > 1 else np.concatenate([x[at: at + w]] * 2)
            pattern = np.concatenate([two[:w], two[:w] if kind == "constant" else two[w:]])
            x[at: at + m * w] = np.tile(pattern, m // 2 + 1)[: m * w]
        at += n
    return x, ref


def width_batch(w, mask, layout="packed"):
    """Every switch length of width w as an item of one batch, all with `mask`."""
    lengths = np.array(switch_lengths(w), np.uint64)
    return lengths, np.full(len(lengths), w, np.uint8), np.full(len(lengths), mask, np.uint8), layout


def mixed_batch(nitems, seed, longest=0):
    """Mixed widths and masks over `nitems` items of 0 .. 4096 bytes, and one item of `longest` bytes in the middle."""
    rs = np.random.RandomState(seed)
    widths = np.array(WIDTHS, np.uint8)[rs.randint(0, 4, nitems)]
    lengths = rs.randint(0, 4097, nitems).astype(np.uint64)
    if longest:
        lengths[nitems // 2] = longest
    masks = np.array([masks_of(int(w))[rs.randint(0, len(masks_of(int(w))))] for w in widths], np.uint8)
    return lengths, widths, masks, LAYOUTS[seed % 3]


# ---- the table of the documents: which candidate wins where ---------------------------------------------------------------------
def table_rows():
    """The nine rows of DESIGN.md section 19 (generator torch.Generator().manual_seed(7); 512 Ki elements, 128 Ki of the 8-byte
    types), cut into items of width * 65536 bytes -> a list of (name, data, base, width, the pick, tie: the pick is a tie)."""
    import torch
    g = torch.Generator().manual_seed(7)
    n, n8 = 512 << 10, 128 << 10

    def randn(count):
        return torch.randn(count, generator=g)

    def bf16(t):
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)

    rows = []
    w = randn(n) * 0.02
    rows.append(("bf16 moved", bf16(w + randn(n) * 1e-4), bf16(w), 2, "subzz", False))
    rows.append(("bf16 unrelated", bf16(randn(n) * 0.02), bf16(randn(n) * 0.02), 2, None, False))
    f = (randn(n) * 0.02).numpy()
    rows.append(("fp32 identical", f.copy(), f, 4, "subzz", True))
    f = randn(n) * 0.02
    rows.append(("fp32 moved", (f + randn(n) * 1e-7).numpy(), f.numpy(), 4, "subzz", False))
    a = torch.sort(torch.randint(0, 1 << 40, (n8,), generator=g)).values.numpy()
    b = torch.sort(torch.randint(0, 1 << 40, (n8,), generator=g)).values.numpy()
    rows.append(("sorted int64", a, b, 8, "delta", False))
    c = torch.randint(0, 1 << 62, (n8,), generator=g).numpy().astype(np.uint64)
    rows.append(("uint64 counters", c + torch.randint(0, 50, (n8,), generator=g).numpy().astype(np.uint64), c, 8, "subzz", True))
    u = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).numpy()
    flip = (torch.rand(n, generator=g) < 0.01).numpy().astype(np.uint8)
    rows.append(("uint8 flipped", u ^ flip, u, 1, "xor", False))
    rows.append(("uint8 unrelated", torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).numpy(), u, 1, None, False))
    rows.append(("zeros", np.zeros(n, np.float32), np.zeros(n, np.float32), 4, None, False))
    return rows


def row_tables(data, width):
    """A row cut into items of width * 65536 bytes -> (bytes, offsets, widths, masks: everything the width may ask for)."""
    x = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    count = -(-len(x) // (width * 65536))
    offs = np.minimum(np.arange(count + 1, dtype=np.uint64) * np.uint64(width * 65536), np.uint64(len(x)))
    return x, offs, np.full(count, width, np.uint8), np.full(count, ts.ALL_OPS if width == 1 else ts.ALL, np.uint8)
