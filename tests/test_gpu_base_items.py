"""Residuals against a base per item on the GPU (include/rcx_base_items.h; csrc/rcx_base_items.hpp) against the numpy statement
(cpprcoder_amd/base_items.py), and against the existing calls on common ground.

rcx_base_items_k spreads units of 16 elements over all items of a class (width, op): a row is 256 units, a workgroup step
RCX_BASE_ROWS(width) rows, what is not a unit goes byte by byte; the items without an op go to rcx_typed_items_k and its scan
kernel as they are.  The batches (tests/base_items_cases.py) sit on both sides of every border of that, with the base spans
in item order, in reverse order and all in one place, at independent offsets of source, base and destination from
(0, 1, 3, 8, 15), every buffer guarded, in four data kinds; then 65 535 to 65 537 items, 8 MiB + 5 bytes in one class, and
37 steps more than the fixed grid has workgroups (33 MiB), where it loops.
"""
import zlib

import numpy as np
import pytest

import base_cases as bcs
import base_items_cases as bc
from cpprcoder_amd import base, base_items as bi, container, rcx, typed_items
from gpu_support import CODERS, Guarded, assert_same_items, ctx, oracle_streams, run_filter  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20261).randint(0, 256, (9 << 20) + 64, dtype=np.uint8)


@pytest.fixture(scope="module")
def cases():
    return bc.kernel_cases()


def run(ctx, join, x, ref, offs, boffs, widths, preds, ops, src_offset=0, base_offset=0, dst_offset=0):
    """gpu_support.run_filter of one base item call over a batch that fills the buffer; the base guarded as well, and unchanged."""
    assert len(offs) == 1 or (int(offs[0]) == 0 and int(offs[-1]) == len(x))
    fn = bi.join_device if join else bi.split_device
    their = Guarded(len(ref), base_offset, ref, salt=5)
    out = run_filter(ctx, lambda src, dst: fn(ctx, src, their.view, offs, boffs, widths, preds, ops, dst),
                     f"base items {'join' if join else 'split'} nitems={len(widths)}", x, src_offset, dst_offset)
    their.check(0, "the base")
    return out


# ---- the kernels against numpy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.KINDS)
def test_split_and_join_against_numpy(ctx, noise, cases, kind):
    assert len(cases) == 30
    for k, case in enumerate(cases):
        x, ref = bc.case_data(case, kind, noise[k:])
        offs, (boffs, _) = bc.offsets_of(case), bc.base_layout(case)
        tables = (offs, boffs, case["widths"], case["preds"], case["ops"])
        y = bi.split_numpy(x, ref, *tables)
        so, bo, do = case["src_offset"], case["base_offset"], case["dst_offset"]
        got = run(ctx, False, x, ref, *tables, so, bo, do)
        bad = np.flatnonzero(got != y)
        assert len(bad) == 0, ("split", case["name"], kind, so, bo, do, bad[:8])
        back = run(ctx, True, y, ref, *tables, do, bo, so)
        bad = np.flatnonzero(back != x)
        assert len(bad) == 0, ("join", case["name"], kind, do, bo, so, bad[:8])


def test_items_inside_a_larger_buffer(ctx, noise):
    """The offsets need not begin at 0 or end with the buffer: exactly [offsets[0], offsets[nitems]) is written."""
    n = 20_000
    x, ref = noise[5: 5 + n], noise[30_000: 36_100]
    offs = np.array([777, 777 + 4 * 1000 + 3, 9000, 9000, 15_001], np.uint64)
    boffs = np.array([1, 0, 0, 0], np.uint64)  # items 0 and 3 overlap in the base
    widths, preds, ops = np.array([4, 2, 8, 1], np.uint8), np.array([0, 1, 0, 0], np.uint8), np.array([2, 0xFF, 1, 0], np.uint8)
    want = bi.split_numpy(x, ref, offs, boffs, widths, preds, ops)
    src, their, dst = Guarded(n, 3, x, salt=1), Guarded(len(ref), 1, ref, salt=5), Guarded(n, 1, salt=2)
    bi.split_device(ctx, src.view, their.view, offs, boffs, widths, preds, ops, dst.view)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(dst.view.cpu().numpy()[777:15_001], want[777:15_001])
    dst.tensor[dst.at + 777: dst.at + 15_001] = dst.before[dst.at + 777: dst.at + 15_001]
    dst.check(0, "split dst outside the items")
    src.check(0, "split src")
    mid, out = Guarded(n, 8, want, salt=3), Guarded(n, 15, salt=4)
    bi.join_device(ctx, mid.view, their.view, offs, boffs, widths, preds, ops, out.view)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(out.view.cpu().numpy()[777:15_001], x[777:15_001])
    out.tensor[out.at + 777: out.at + 15_001] = out.before[out.at + 777: out.at + 15_001]
    out.check(0, "join dst outside the items")
    their.check(0, "the base")


# ---- common ground -------------------------------------------------------------------------------------------------------------
def test_without_ops_it_is_the_typed_item_calls(ctx, noise, cases):
    """ops = None, no base and no base offsets: byte for byte what rcx_typed_items_* write."""
    for case in cases:
        if case["name"] not in ("mixed small", "mixed many", "none with a base", "empty runs"):
            continue
        x = noise[: int(case["lengths"].sum())]
        offs, widths, preds = bc.offsets_of(case), case["widths"], np.where(case["ops"] == bc.NO_BASE, case["preds"], 0).astype(np.uint8)
        want = run_filter(ctx, lambda s, d: typed_items.split_device(ctx, s, offs, widths, preds, d), "typed split", x, 1, 3)
        got = run_filter(ctx, lambda s, d: bi.split_device(ctx, s, None, offs, None, widths, preds, None, d), "base items split", x, 1, 3)
        assert np.array_equal(got, want), case["name"]
        back = run_filter(ctx, lambda s, d: typed_items.join_device(ctx, s, offs, widths, preds, d), "typed join", want, 3, 8)
        got = run_filter(ctx, lambda s, d: bi.join_device(ctx, s, None, offs, None, widths, preds, None, d), "base items join", want, 3, 8)
        assert np.array_equal(got, back) and np.array_equal(back, x), case["name"]


@pytest.mark.parametrize("width", bc.WIDTHS)
@pytest.mark.parametrize("op", bc.OPS)
def test_superblock_cut_items_equal_the_base_calls(ctx, noise, width, op):
    for block in bcs.BLOCKS:  # 16, 48, 100, 4096, 4112
        n = 3 * width * block + (37 if block > 37 else 5)
        x, ref = noise[11: 11 + n], noise[100_000: 100_000 + n]
        lengths, widths, ops = bc.superblock_items(n, width, block, op)
        offs = rcx.item_offsets(lengths)
        assert len(lengths) == 4
        their = Guarded(n, 15, ref, salt=5)
        want = run_filter(ctx, lambda s, d: base.split_device(ctx, s, their.view, width, block, op, d), "base split", x, 1, 3)
        assert np.array_equal(want, base.split_numpy(x, ref, width, block, op))
        got = run_filter(ctx, lambda s, d: bi.split_device(ctx, s, their.view, offs, offs[:-1], widths, None, ops, d), "base items split", x, 1, 3)
        assert np.array_equal(got, want), block
        back = run_filter(ctx, lambda s, d: base.join_device(ctx, s, their.view, width, block, op, d), "base join", want, 3, 1)
        got = run_filter(ctx, lambda s, d: bi.join_device(ctx, s, their.view, offs, offs[:-1], widths, None, ops, d), "base items join", want, 3, 1)
        assert np.array_equal(got, back) and np.array_equal(back, x), block
        their.check(0, "the base")


# ---- many items, and grids that loop -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(noise):
    """65 537 items of 0 to 40 bytes, every kind in turn, base spans packed; the expectation once: fewer items are a prefix of it."""
    rs = np.random.RandomState(66)
    lengths = rs.randint(0, 41, 65537).astype(np.uint64)
    pick = rs.randint(0, len(bc.ITEM_KINDS), 65537)
    widths, preds, ops = (np.array([bc.ITEM_KINDS[k][j] for k in pick], np.uint8) for j in range(3))
    case = {"lengths": lengths, "widths": widths, "preds": preds, "ops": ops, "layout": "packed"}
    offs, (boffs, nbase) = rcx.item_offsets(lengths), bc.base_layout(case)
    x, ref = noise[: int(offs[-1])], noise[(4 << 20): (4 << 20) + nbase]
    return widths, preds, ops, offs, boffs, x, ref, bi.split_numpy(x, ref, offs, boffs, widths, preds, ops)


@pytest.mark.parametrize("nitems", (65535, 65536, 65537))
def test_item_counts_around_two_to_the_sixteen(ctx, many, nitems):
    widths, preds, ops, offs, boffs, x, ref, y = many
    n = int(offs[nitems])
    tables = (offs[: nitems + 1], boffs[:nitems], widths[:nitems], preds[:nitems], ops[:nitems])
    assert np.array_equal(run(ctx, False, x[:n], ref, *tables, 1, 3, 8), y[:n])
    assert np.array_equal(run(ctx, True, y[:n], ref, *tables, 3, 8, 0), x[:n])


@pytest.mark.parametrize("width,op", [(1, bi.SUBZZ), (2, bi.SUB), (4, bi.XOR), (8, bi.SUBZZ)])
def test_eight_mebibytes_and_five_bytes_in_one_class(ctx, noise, width, op):
    """Items of 0 bytes to a MiB and a tail, one class: 256 workgroup steps of 32 KiB, rows that cross items, rests of every length."""
    n = (8 << 20) + 5
    sizes = [(1 << 20) + 3, 65536, 4 * 4099, 100_000, 8 * 65536 + 7, 33, 2 * 70_000 + 1, 0, 12_345]
    lengths, total = [], 0
    while total < n:
        lengths.append(min(sizes[len(lengths) % len(sizes)], n - total))
        total += lengths[-1]
    lengths = np.array(lengths, np.uint64)
    widths, ops = np.full(len(lengths), width, np.uint8), np.full(len(lengths), op, np.uint8)
    offs = rcx.item_offsets(lengths)
    boffs = ((offs[-1] - offs[1:]) // np.uint64(2)).astype(np.uint64)  # spans that overlap, in reverse order
    x, ref = noise[3: 3 + n], noise[40: 40 + n]
    y = bi.split_numpy(x, ref, offs, boffs, widths, None, ops)
    assert np.array_equal(run(ctx, False, x, ref, offs, boffs, widths, None, ops, 0, 1, 0), y)
    assert np.array_equal(run(ctx, True, y, ref, offs, boffs, widths, None, ops, 0, 1, 0), x)


def test_more_steps_than_the_grid_has_workgroups(ctx, noise):
    """The fixed grid is four workgroups a compute unit (read from the device) and a step is 32 KiB in every class: 32 MiB are the
    1024 steps that 256 compute units take in one go, so the buffer is 37 steps more than the grid, 33.2 MiB there, and the step
    loop goes round; in items of three steps and 7 elements and a byte, all against ONE span."""
    steps = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    lengths = np.array([3 * 32768 + 2 * 7 + 1] * (steps // 3) + [32768 * (steps % 3) + 2], np.uint64)
    assert int(lengths.sum()) <= (36 << 20)
    widths, ops = np.full(len(lengths), 2, np.uint8), np.full(len(lengths), bi.SUBZZ, np.uint8)
    offs, boffs = rcx.item_offsets(lengths), np.zeros(len(lengths), np.uint64)
    x, ref = np.resize(noise, int(offs[-1])), noise[77: 77 + int(lengths.max())]
    y = bi.split_numpy(x, ref, offs, boffs, widths, None, ops)
    assert np.array_equal(run(ctx, False, x, ref, offs, boffs, widths, None, ops, 1, 3, 0), y)
    assert np.array_equal(run(ctx, True, y, ref, offs, boffs, widths, None, ops, 0, 3, 3), x)


def test_host_buffer_calls(ctx, noise, cases):
    names = ("mixed small", "empty runs", "large and small", "only empty", "many on one span", "reverse order", "none with a base")
    for case in [c for c in cases if c["name"] in names]:
        x, ref = bc.case_data(case, "random", noise)
        offs, (boffs, _) = bc.offsets_of(case), bc.base_layout(case)
        tables = (offs, boffs, case["widths"], case["preds"], case["ops"])
        y = bi.split(ctx, x, ref, *tables)
        assert y == bi.split_numpy(x, ref, *tables).tobytes(), case["name"]
        assert bi.join(ctx, y, ref, *tables) == x.tobytes(), case["name"]
    x, ref = noise[:3000], noise[5000:9000]
    offs, boffs, widths = np.array([100, 1100, 2103], np.uint64), np.array([3000, 1500], np.uint64), np.array([8, 2], np.uint8)
    y = bi.split(ctx, x, ref, offs, boffs, widths, None, [1, 2])  # the copies begin at the first item and at the lowest span
    assert y == bi.split_numpy(x, ref, offs, boffs, widths, None, [1, 2]).tobytes() and bi.join(ctx, y, ref, offs, boffs, widths, None, [1, 2]) == x.tobytes()
    assert bi.split(ctx, x, None, offs, None, widths, [1, 2], None) == typed_items.split(ctx, x, offs, widths, [1, 2])


def test_a_side_stream(ctx, noise, cases):
    case = next(c for c in cases if c["name"] == "mixed many")
    x, ref = bc.case_data(case, "random", noise)
    offs, (boffs, _) = bc.offsets_of(case), bc.base_layout(case)
    tables = (offs, boffs, case["widths"], case["preds"], case["ops"])
    y = bi.split_numpy(x, ref, *tables)
    side = torch.cuda.Stream()
    src, their, dst, out = Guarded(len(x), 1, x, salt=1), Guarded(len(ref), 3, ref, salt=5), Guarded(len(x), 8, salt=2), Guarded(len(x), 0, salt=3)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        bi.split_device(ctx, src.view, their.view, *tables, dst.view, stream=side)
        bi.join_device(ctx, dst.view, their.view, *tables, out.view, stream=side)
    side.synchronize()
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(dst.view.cpu().numpy(), y) and np.array_equal(out.view.cpu().numpy(), x)
    for buf in (src, their):
        buf.check(0, "an input")
    dst.check(len(x), "dst")
    out.check(len(x), "out")


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(ctx, noise):
    L, h = bi.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    src, their, dst = Guarded(n, 0, noise[:n], salt=1), Guarded(n, 0, noise[n: 2 * n], salt=5), Guarded(n, 0, salt=2)
    room = Guarded(3 * n, 0, noise[: 3 * n], salt=3)  # one allocation for the overlapping and the adjacent ranges
    s, b, d, r = src.view.data_ptr(), their.view.data_ptr(), dst.view.data_ptr(), room.view.data_ptr()
    host_out = np.full(n, 0xA5, np.uint8)

    def tables(offs, boffs, widths, preds, ops):
        t = [np.array(offs, np.uint64), None if boffs is None else np.array(boffs, np.uint64), np.array(widths, np.uint8),
             None if preds is None else np.array(preds, np.uint8), None if ops is None else np.array(ops, np.uint8)]
        return t, tuple(None if a is None else a.ctypes.data for a in t) + (len(widths),)

    good, g = tables([0, 1000, n], [0, 1000], [4, 2], [1, 0], [0xFF, 2])
    big = (1 << 24) - 256
    bad_tables = [tables([0, 1000, n], [0, 0], [4, 3], None, [0, 0]), tables([0, 1000, n], [0, 0], [4, 2], [3, 0], None),      # rcx_typed_items.h's: a width, a predictor
                  tables([0, 1000, n], [0, 0], [1, 2], [1, 0], None), tables([0, 1000, 999], [0, 0], [4, 2], None, [0, 0]),     # ... width 1, decreasing offsets
                  tables([0, 8 * (big + 1)], [0], [8], None, [0]),                                                             # ... a sub-item above the limit
                  tables([0, 1000, n], [0, 0], [4, 2], None, [3, 0]), tables([0, 1000, n], [0, 0], [4, 2], None, [0, 0xFE]),    # an op
                  tables([0, 0, 0], [0, 0], [4, 2], None, [9, 0]),                                                            # ... also with nothing to do
                  tables([0, 1000, n], [0, 0], [4, 2], [1, 0], [1, 0xFF]), tables([0, 0, 0], [0, 0], [4, 2], [0, 2], [0xFF, 0]),  # a predictor AND an op
                  tables([0, 1000, n], None, [4, 2], None, [0xFF, 1]),                                                        # an op in use and no base offsets
                  tables([0, 1000, n], [0, (1 << 64) - 100], [4, 2], None, [0xFF, 1])]                                         # a span around 2^64
    for fn in (L.rcx_base_items_split_device, L.rcx_base_items_join_device):
        assert fn(h, s, b, None, None, None, None, None, 0, d, stream) == rcx.OK and fn(h, None, None, None, None, None, None, None, 0, None, stream) == rcx.OK
        empty, e = tables([5, 5, 5], None, [2, 1], None, [2, 0])
        assert fn(h, None, None, *e, None, stream) == rcx.OK and fn(h, s, b, *e, d, stream) == rcx.OK  # no bytes: no base offsets needed either
        for keep, t in bad_tables:
            assert fn(h, s, b, *t, d, stream) == rcx.E_ARG, keep
        for st in (fn(None, s, b, *g, d, stream), fn(h, None, b, *g, d, stream), fn(h, s, b, *g, None, stream), fn(h, s, None, *g, d, stream),  # null pointers
                   fn(h, s, b, None, *g[1:], d, stream), fn(h, s, b, g[0], g[1], None, *g[3:], d, stream),                                  # null tables
                   fn(h, r, b, *g, r, stream), fn(h, r, b, *g, r + 1, stream), fn(h, r + 1, b, *g, r, stream),                               # dst over src
                   fn(h, r, b, *g, r + n - 1, stream), fn(h, r + n - 1, b, *g, r, stream),
                   fn(h, s, r, *g, r, stream), fn(h, s, r + 1000, *g, r, stream), fn(h, s, r - 999, *g, r + n - 1000, stream),               # dst over the hull
                   fn(h, s, r + n - 1001, *g, r, stream)):                                                                              # (the hull is 1000 .. 4096)
            assert st == rcx.E_ARG
    hull, hh = tables([0, 100, 200, 300], [0, 0, 3000], [1, 1, 1], None, [0, 0xFF, 0])  # spans 0..100 and 3000..3100: the gap is part of the hull
    for fn in (L.rcx_base_items_split_device, L.rcx_base_items_join_device):
        assert fn(h, s, r, *hh, r + 1000, stream) == rcx.E_ARG
    for fn in (L.rcx_base_items_split, L.rcx_base_items_join):
        p = noise.ctypes.data
        for keep, t in bad_tables:
            assert fn(h, p, p + 8192, n, *t, host_out.ctypes.data) == rcx.E_ARG, keep
        for st in (fn(h, None, p + 8192, n, *g, host_out.ctypes.data), fn(h, p, p + 8192, n, *g, None), fn(h, p, None, n, *g, host_out.ctypes.data),
                   fn(h, p, p + 8192, n, *g, p + 100), fn(h, p, host_out.ctypes.data, n, *g, host_out.ctypes.data),
                   fn(h, p, p + 8192, n - 1, *g, host_out.ctypes.data),  # the last span ends past base_bytes
                   fn(None, p, p + 8192, n, *g, host_out.ctypes.data)):
            assert st == rcx.E_ARG
        assert fn(h, None, None, 0, None, None, None, None, None, 0, None) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for buf, what in ((src, "src"), (their, "base"), (dst, "dst"), (room, "room")):
        buf.check(0, what)  # not a byte changed anywhere
    assert bool((host_out == 0xA5).all())
    assert bi.check(*good) == rcx.OK and bi.hull(*good) == (1000, n) and bi.hull(*hull) == (0, 3100)
    assert all(bi.check(*keep) == rcx.E_ARG for keep, _ in bad_tables)


def test_touching_ranges_are_apart(ctx, noise):
    """The second third of an allocation from its first with the base in the third, and the third from the second with the base in
    the first: source, destination and hull touch and are accepted."""
    L, h, n = bi.lib(), ctx._h, 4096
    stream = torch.cuda.current_stream().cuda_stream
    room = Guarded(3 * n, 0, noise[: 3 * n], salt=3)
    r = room.view.data_ptr()
    offs, boffs = np.array([0, 1000, n], np.uint64), np.array([0, 0], np.uint64)
    widths, ops = np.array([4, 2], np.uint8), np.array([1, 2], np.uint8)
    g = (offs.ctypes.data, boffs.ctypes.data, widths.ctypes.data, None, ops.ctypes.data, 2)
    first = noise[:n].copy()
    y = bi.split_numpy(first, noise[2 * n: 3 * n], offs, boffs, widths, None, ops)
    assert L.rcx_base_items_split_device(h, r, r + 2 * n, *g, r + n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[:n], first) and np.array_equal(got[n: 2 * n], y) and np.array_equal(got[2 * n:], noise[2 * n: 3 * n])
    z = bi.join_numpy(y, first, offs, boffs, widths, None, ops)
    assert L.rcx_base_items_join_device(h, r + n, r, *g, r + 2 * n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[:n], first) and np.array_equal(got[n: 2 * n], y) and np.array_equal(got[2 * n:], z)
    room.check(3 * n, "room")


def test_the_tables_count_as_scratch(ctx, noise):
    """rcx_ctx_scratch_bytes counts the item tables: after a call with 20 000 items the context holds at least their 20 bytes each."""
    before = ctx.scratch_bytes()
    nitems = 20_000
    lengths = np.full(nitems, 8, np.uint64)
    offs = rcx.item_offsets(lengths)
    x, ref = noise[: 8 * nitems], noise[8 * nitems: 16 * nitems]
    widths, ops = np.full(nitems, 4, np.uint8), np.full(nitems, 1, np.uint8)
    assert np.array_equal(run(ctx, False, x, ref, offs, offs[:-1], widths, None, ops), bi.split_numpy(x, ref, offs, offs[:-1], widths, None, ops))
    assert ctx.scratch_bytes() >= max(before, 28 * nitems)


# ---- containers ------------------------------------------------------------------------------------------------------------------
def container_items():
    """(bytes, base or None, width, op by name or None, predictor by name or None): weights that moved a little, a frozen buffer,
    bytes, counters, a new buffer, sorted keys with a predictor, nothing, less than an element."""
    rng = np.random.default_rng(4)
    w = (rng.standard_normal(2500) * 0.02).astype(np.float32)
    moved, before = bcs.bf16_bytes(w + rng.standard_normal(2500) * 1e-4), bcs.bf16_bytes(w)
    frozen = rng.standard_normal(700).astype(np.float32).view(np.uint8)
    text, text2 = np.frombuffer(b"plain bytes, thirty-three of them", np.uint8), np.frombuffer(b"plain bytes: thirty-four of them", np.uint8)
    now, then = bcs.counter_pair(1 << 10)
    keys = np.sort(rng.integers(0, 1 << 40, 1000)).astype("<i8").view(np.uint8)
    return [(moved, before, 2, "subzz", None), (frozen, frozen.copy(), 4, "xor", None), (text[:32], text2[:32], 1, "sub", None), (now[:8 * 1000 + 5], then[:8 * 1000 + 5], 8, "sub", None),
            (bcs.bf16_bytes(rng.standard_normal(999)), None, 2, None, None), (keys, None, 8, None, "delta"), (np.zeros(0, np.uint8), np.zeros(0, np.uint8), 4, "sub", None),
            (np.arange(7, dtype=np.uint8), np.arange(7, dtype=np.uint8)[::-1].copy(), 8, "subzz", None), (keys[:4003], keys[3997:8000], 4, "subzz", None)]


def pack_args(items):
    return ([it[0] for it in items], [it[1] for it in items]), dict(widths=[it[2] for it in items], ops=[it[3] for it in items], predict=[it[4] for it in items])


@pytest.fixture(scope="module")
def packed_sub_items():
    """The items, their tables, and the sub-items of the numpy residual."""
    items = container_items()
    widths = np.array([it[2] for it in items], np.uint8)
    ops = np.array([bi.NO_BASE if it[3] is None else container.BASE_OPS[it[3]] for it in items], np.uint8)
    preds = np.array([container.PREDICTORS[it[4]] for it in items], np.uint8)
    lengths = np.array([len(it[0]) for it in items], np.uint64)
    offs = rcx.item_offsets(lengths)
    boffs = rcx.item_offsets(np.where(ops != bi.NO_BASE, lengths, 0))
    ref = np.concatenate([it[1] for it, op in zip(items, ops) if op != bi.NO_BASE])
    y = bi.split_numpy(np.concatenate([it[0] for it in items]), ref, offs, boffs[:-1], widths, preds, ops)
    sub = typed_items.sub_offsets_numpy(offs, widths)
    return items, widths, preds, ops, [y[int(sub[k]): int(sub[k + 1])] for k in range(len(sub) - 1)]


@pytest.mark.parametrize("coder", CODERS)
def test_sub_item_streams_are_the_oracles_of_the_numpy_residual(ctx, oracle, packed_sub_items, coder):
    items, widths, preds, ops, subs = packed_sub_items
    want = oracle_streams(oracle, subs, coder)
    raw = [it[0].tobytes() for it in items]
    args, kw = pack_args(items)
    for checksum in (False, True):
        blob = container.pack_delta_items(*args, **kw, coder=coder, ctx=ctx, checksum=checksum, directory=b"carried")
        c = container.parse_delta_items(blob)
        inner = c["inner"]
        assert (inner["coder"], c["nitems"], inner["nsub"], inner["directory"]) == (coder, len(items), int(widths.sum()), b"carried")
        assert list(c["ops"]) == list(ops) and list(inner["widths"]) == list(widths) and list(inner["preds"]) == list(preds)
        assert list(c["base_crcs"]) == [zlib.crc32(it[1].tobytes()) if op != bi.NO_BASE and len(it[0]) else 0 for it, op in zip(items, ops)]
        assert_same_items(inner["payload"], inner["offsets"], want, (coder, checksum))
        if checksum:
            assert list(inner["crcs"]) == [zlib.crc32(s.tobytes()) if len(s) else 0 for s in subs]
        assert container.unpack_delta_items(blob, args[1], ctx=ctx) == raw
        # an RCXJ reader that skips the prefix gets the residuals, and the data of the items without a base
        plain = container.unpack_typed_items(blob[c["inner_at"]:], ctx=ctx)
        assert plain[4] == raw[4] and plain[5] == raw[5] and plain[0] != raw[0] and not any(plain[1])


def test_round_trips_with_options_and_sources(ctx):
    items = container_items()
    raw = [it[0].tobytes() for it in items]
    args, kw = pack_args(items)
    want = container.pack_delta_items(*args, **kw, ctx=ctx, checksum=True)
    for convert in (lambda a: a.tobytes(), lambda a: a, lambda a: torch.from_numpy(a.copy()), lambda a: torch.from_numpy(a.copy()).cuda()):
        given = [convert(it[0]) for it in items], [None if it[1] is None else convert(it[1]) for it in items]
        assert container.pack_delta_items(*given, **kw, ctx=ctx, checksum=True) == want  # where the bytes lie changes nothing
        assert container.unpack_delta_items(want, given[1], ctx=ctx) == raw
    for options in (dict(stored=True), dict(stored=0.5, checksum=True), dict(base_check=False), dict(coder=2, checksum=True, stored=True)):
        blob = container.pack_delta_items(*args, **kw, ctx=ctx, **options)
        c = container.parse_delta_items(blob)
        assert (c["base_crcs"] is None) == (options.get("base_check") is False)
        if "stored" in options:
            assert c["inner"].get("stored") is not None and c["inner"]["stored"].any()  # the bf16 mantissa planes of the new buffer do not shrink
        assert container.unpack_delta_items(blob, args[1], ctx=ctx) == raw and container.unpack_delta_items(blob, args[1], ctx=ctx, verify=False) == raw
    # one op for all that have a base; predict for those that have none; "auto" measures only those
    blob = container.pack_delta_items(*args, widths=kw["widths"], ops="sub", predict="auto", ctx=ctx)
    c = container.parse_delta_items(blob)
    assert list(c["ops"]) == [1, 1, 1, 1, 0xFF, 0xFF, 1, 1, 1] and list(c["inner"]["preds"]) == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert container.unpack_delta_items(blob, args[1], ctx=ctx) == raw
    # a base that is there and not used
    blob = container.pack_delta_items(*args, widths=kw["widths"], ops=[None] * 9, predict=kw["predict"], ctx=ctx)
    assert blob[container.parse_delta_items(blob)["inner_at"]:] == container.pack_typed_items(args[0], kw["widths"], kw["predict"], 0, ctx)
    assert container.unpack_delta_items(blob, [None] * 9, ctx=ctx) == raw


def test_picks_decode_and_verify_only_their_items(ctx, monkeypatch):
    items = container_items()
    raw = [it[0].tobytes() for it in items]
    args, kw = pack_args(items)
    blob = container.pack_delta_items(*args, **kw, ctx=ctx, checksum=True)
    c = container.parse_delta_items(blob)
    decoded, verified, real_decode, real_verify = [], [], ctx.decode_items_device, ctx.verify_items_device

    def decode_items_device(*a, pick=None, **k):
        decoded.append([int(s) for s in pick])
        return real_decode(*a, pick=pick, **k)

    def verify_items_device(src, offs, expected, **k):
        verified.append((int(src.numel()), [int(v) for v in np.diff(np.asarray(offs).astype(np.int64))]))
        return real_verify(src, offs, expected, **k)

    monkeypatch.setattr(ctx, "decode_items_device", decode_items_device)
    monkeypatch.setattr(ctx, "verify_items_device", verify_items_device)
    first = [int(v) for v in c["inner"]["sub_first"]]
    for pick in ([0], [3, 0], [8, 7, 6, 5, 4, 3, 2, 1, 0], [1, 1, 3, 1], [2], [5], [4, 5], [6, 2, 6]):
        before = len(verified)
        bases = [args[1][k] if k in pick else None for k in range(9)]  # only the picks' bases are there
        assert container.unpack_delta_items(blob, bases, pick, ctx) == [raw[k] for k in pick], pick
        assert decoded[-1] == [s for k in pick for s in range(first[k], first[k + 1])], pick  # the picks' sub-items and no others
        spans = [len(raw[k]) if items[k][3] is not None else 0 for k in pick]
        if sum(spans):  # the guard: the picks' bases back to back, nothing for a pick without one; then the split text
            assert len(verified) == before + 2 and verified[before] == (sum(spans), spans), pick
        else:
            assert len(verified) == before + 1, pick
    calls = len(decoded)
    assert container.unpack_delta_items(blob, [None] * 9, [], ctx) == [] and container.unpack_delta_items(blob, [None] * 9, [6], ctx) == [b""] and len(decoded) == calls
    before = len(verified)
    assert container.unpack_delta_items(blob, args[1], None, ctx, verify=False) == raw and len(verified) == before
    with pytest.raises(container.ContainerError):
        container.unpack_delta_items(blob, args[1], [9], ctx)
    with pytest.raises(container.ContainerError, match="item 3"):
        container.unpack_delta_items(blob, [None] * 9, [4, 3], ctx)  # a missing base


def state_dicts():
    torch.manual_seed(12)
    w = torch.randn(300, 70) * 0.02
    named = {"layer.weight": (w + torch.randn(300, 70) * 1e-4).to(torch.bfloat16), "layer.norm": torch.randn(1000) * 0.02 + 1,
             "table": torch.sort(torch.randint(0, 10 ** 9, (5000,)))[0], "mask": torch.rand(4099) < 0.2, "bytes": torch.randint(0, 256, (3, 1000), dtype=torch.uint8),
             "empty": torch.zeros(0, 4, dtype=torch.float32), "scalar": torch.tensor(3.25, dtype=torch.float32), "new.bias": torch.randn(17, dtype=torch.float16),
             "counts": torch.randint(0, 1 << 40, (6000,)), "reshaped": torch.randn(20, 30)}
    before = {"layer.weight": w.to(torch.bfloat16), "layer.norm": named["layer.norm"].clone(), "mask": named["mask"] ^ (torch.rand(4099) < 0.01),
              "bytes": named["bytes"].clone(), "empty": torch.zeros(0, 4, dtype=torch.float32), "scalar": torch.tensor(3.0, dtype=torch.float32),
              "counts": named["counts"] - torch.randint(0, 50, (6000,)), "reshaped": torch.randn(30, 20), "table": named["table"].to(torch.int32), "gone": torch.zeros(5)}
    return named, before


BASED = ("layer.weight", "layer.norm", "mask", "bytes", "scalar", "counts")  # in the base with the same dtype and shape, and with bytes


@pytest.mark.parametrize("source", ("cpu", "cuda", "numpy"))
@pytest.mark.parametrize("device", ("cpu", "cuda"))
def test_a_state_dict_round_trips_against_the_one_before(ctx, monkeypatch, source, device):
    named, before = state_dicts()
    kw = dict(block=4096, predict={"table": "delta"}, ctx=ctx, checksum=True)
    want = container.pack_tensors_delta(named, before, **kw)

    def given(d):
        return {k: v.cuda() for k, v in d.items()} if source == "cuda" else {k: (v.numpy() if v.dtype != torch.bfloat16 else v) for k, v in d.items()} if source == "numpy" else d

    blob = container.pack_tensors_delta(given(named), given(before), **kw)
    assert blob == want  # where the bytes lie changes nothing
    c = container.parse_delta_items(blob)
    entries = {e["name"]: e for e in container.parse_tensor_directory(c["inner"]["directory"], c["nitems"])}
    assert list(entries) == list(named)
    for name, e in entries.items():
        items = slice(e["first"], e["first"] + e["count"])
        assert set(c["ops"][items]) <= ({2} if name in BASED + ("empty",) else {0xFF}), name
        assert set(c["inner"]["preds"][items]) <= ({1} if name == "table" else {0}), name
    if device == "cuda":  # without a download: nothing of the result passes through the host
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self: (_ for _ in ()).throw(AssertionError("a download")))
    back = container.unpack_tensors_delta(blob, given(before) if device == "cpu" else {k: v.cuda() for k, v in before.items()}, device=device, ctx=ctx)
    monkeypatch.undo()
    assert list(back) == list(named)
    for name, t in named.items():
        assert back[name].device.type == device and back[name].dtype == t.dtype and back[name].shape == t.shape, name
        assert torch.equal(back[name].cpu(), t), name


def test_names_decode_only_their_items_and_need_only_their_bases(ctx, monkeypatch):
    named, before = state_dicts()
    blob = container.pack_tensors_delta(named, before, block=4096, ctx=ctx, checksum=True)
    c = container.parse_delta_items(blob)
    by_name = {e["name"]: e for e in container.parse_tensor_directory(c["inner"]["directory"], c["nitems"])}
    seen, guarded, real, real_verify = [], [], ctx.decode_items_device, ctx.verify_items_device

    def decode_items_device(*a, pick=None, **kw):
        seen.append(len(pick))
        return real(*a, pick=pick, **kw)

    def verify_items_device(src, offs, expected, **kw):
        guarded.append(int(src.numel()))
        return real_verify(src, offs, expected, **kw)

    monkeypatch.setattr(ctx, "decode_items_device", decode_items_device)
    monkeypatch.setattr(ctx, "verify_items_device", verify_items_device)
    for names in (["table"], ["scalar", "layer.weight"], ["scalar", "empty"], ["mask"], ["new.bias", "counts"]):
        at = len(guarded)
        back = container.unpack_tensors_delta(blob, {n: before[n] for n in names if n in before}, names=names, ctx=ctx)  # only their bases
        assert list(back) == names and all(torch.equal(back[n], named[n]) for n in names)
        assert seen[-1] == sum(by_name[n]["count"] * named[n].element_size() for n in names), names  # streams handed to the decode call
        base_bytes = sum(named[n].numel() * named[n].element_size() for n in names if n in BASED)
        assert guarded[at:] == ([base_bytes] if base_bytes else []) + [sum(named[n].numel() * named[n].element_size() for n in names)], names
    calls = len(seen)
    assert list(container.unpack_tensors_delta(blob, {}, names=["empty"], ctx=ctx)) == ["empty"] and len(seen) == calls  # nothing to decode
    with pytest.raises(container.ContainerError):
        container.unpack_tensors_delta(blob, before, names=["nobody"], ctx=ctx)


def test_a_flipped_base_byte_names_its_item_and_its_tensor(ctx):
    named, before = state_dicts()
    blob = container.pack_tensors_delta(named, before, block=4096, ctx=ctx)
    c = container.parse_delta_items(blob)
    by_name = {e["name"]: e for e in container.parse_tensor_directory(c["inner"]["directory"], c["nitems"])}
    with_op = np.flatnonzero((c["ops"] != 0xFF) & (c["inner"]["lengths"] > 0))
    owner = {k: n for n, e in by_name.items() for k in range(e["first"], e["first"] + e["count"])}
    for item in (int(with_op[0]), int(with_op[len(with_op) // 2]), int(with_op[-1])):  # the first, a middle and the last item with a base
        name = owner[item]
        e = by_name[name]
        bad = dict(before)
        flat = before[name].clone().reshape(-1).view(torch.uint8)
        at = int(c["inner"]["lengths"][e["first"]: item].sum()) + int(c["inner"]["lengths"][item]) - 1  # the item's last byte
        flat[at] ^= 0x40
        bad[name] = flat.view(before[name].dtype).reshape(before[name].shape)
        with pytest.raises(container.BaseItemMismatchError) as err:
            container.unpack_tensors_delta(blob, bad, ctx=ctx)
        assert (err.value.index, err.value.name) == (item, name) and repr(name) in str(err.value) and f"item {item}" in str(err.value)
        with pytest.raises(container.BaseMismatchError):
            container.unpack_tensors_delta(blob, bad, names=["table", name], ctx=ctx)
        others = [n for n in named if n != name]
        back = container.unpack_tensors_delta(blob, bad, names=others, ctx=ctx)  # a base that was not asked for is not checked
        assert all(torch.equal(back[n], named[n]) for n in others)
        got = container.unpack_tensors_delta(blob, bad, ctx=ctx, verify=False)  # nobody asked: wrong elements, and no error
        assert not torch.equal(got[name], named[name]) and all(torch.equal(got[n], named[n]) for n in others)
        # the same through the item call, which has no names
        items = [named[n] for n in named]
        raw = container.pack_delta_items([named[name]], [before[name]], ctx=ctx)
        with pytest.raises(container.BaseItemMismatchError) as err:
            container.unpack_delta_items(raw, [bad[name]], ctx=ctx)
        assert (err.value.index, err.value.name) == (0, None) and len(items) == len(named)
    unguarded = container.pack_tensors_delta(named, before, block=4096, ctx=ctx, base_check=False)
    assert len(unguarded) == len(blob) - 4 * c["nitems"] and container.parse_delta_items(unguarded)["base_crcs"] is None
    got = container.unpack_tensors_delta(unguarded, bad, ctx=ctx)  # no table, no guard
    assert not torch.equal(got[name], named[name])
    assert all(torch.equal(v, named[n]) for n, v in container.unpack_tensors_delta(unguarded, before, ctx=ctx).items())


def test_a_missing_or_misshaped_base_tensor(ctx):
    named, before = state_dicts()
    blob = container.pack_tensors_delta(named, before, block=4096, ctx=ctx)
    for bad in ({k: v for k, v in before.items() if k != "counts"}, dict(before, counts=before["counts"][:5999]), dict(before, mask=before["mask"].to(torch.int16))):
        with pytest.raises(container.ContainerError) as err:
            container.unpack_tensors_delta(blob, bad, ctx=ctx)
        assert not isinstance(err.value, container.BaseMismatchError)
    ok = container.unpack_tensors_delta(blob, {k: v for k, v in before.items() if k != "counts"}, names=["mask", "table"], ctx=ctx)  # ... if it is needed
    assert torch.equal(ok["mask"], named["mask"])
    # an op dict: only the names it gives get their base; one whose base is missing or of another shape or dtype is refused
    blob = container.pack_tensors_delta(named, before, block=4096, op={"counts": "sub", "mask": "xor", "layer.norm": None}, ctx=ctx)
    c = container.parse_delta_items(blob)
    by_name = {e["name"]: e for e in container.parse_tensor_directory(c["inner"]["directory"], c["nitems"])}
    assert {n: sorted(set(c["ops"][e["first"]: e["first"] + e["count"]])) for n, e in by_name.items() if e["count"]} == {
        n: [1] if n == "counts" else [0] if n == "mask" else [0xFF] for n in named if n != "empty"}
    back = container.unpack_tensors_delta(blob, {"counts": before["counts"], "mask": before["mask"]}, ctx=ctx)
    assert all(torch.equal(back[n], named[n]) for n in named)
    for op in ({"new.bias": "sub"}, {"reshaped": "sub"}, {"table": "xor"}):
        with pytest.raises(container.ContainerError):
            container.pack_tensors_delta(named, before, block=4096, op=op, ctx=ctx)


@pytest.mark.parametrize("width", bc.WIDTHS)
def test_one_tensor_carries_the_payload_of_pack_delta(ctx, width):
    block = 4096
    dtype = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[width]
    torch.manual_seed(width)
    before = torch.randint(0, 200, (3 * block,)).to(dtype)  # whole superblocks: there the blocks of the inner RCXT are the planes
    t = (before + torch.randint(-3, 4, (3 * block,)).to(dtype)).to(dtype)
    for op, checksum in (("subzz", False), ("xor", True)):
        delta = container.parse_delta(container.pack_delta(t, before, None, block, 0, ctx, checksum=checksum, op=op))
        blob = container.pack_tensors_delta({"t": t}, {"t": before}, block=block, op=op, ctx=ctx, checksum=checksum)
        c = container.parse_delta_items(blob)
        inner = c["inner"]
        assert c["nitems"] == 3 and inner["nsub"] == delta["inner"]["nblocks"] == 3 * width and list(c["ops"]) == [container.BASE_OPS[op]] * 3
        assert np.array_equal(inner["payload"], delta["inner"]["payload"]) and np.array_equal(inner["offsets"], delta["inner"]["offsets"])  # the same streams
        if checksum:
            assert np.array_equal(inner["crcs"], delta["inner"]["crcs"])
        assert torch.equal(container.unpack_tensors_delta(blob, {"t": before}, ctx=ctx)["t"], t)
