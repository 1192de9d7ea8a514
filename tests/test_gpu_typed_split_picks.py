"""rcx_typed_split_picks_device on the GPU (include/rcx_typed_split_picks.h): the typed split per item whose positions, lengths,
widths, predictors and count are read from device memory, planned by kernels, capturable in a graph; and
container.pack_typed_items_device / PackedTypedItems on top of it and of rcx_encode_picks_device.  Expected bytes are
typed_items.split_numpy's and the host-planned call's; what is latched and kept is what cpprcoder_amd/typed_split_picks.py's numpy
model of the planner says.  Every output buffer is guarded and compared whole.  Nothing here reads the reference's tree."""
import numpy as np
import pytest

import typed_items_cases as tc
from cpprcoder_amd import container, encode_picks, picks, rcx, typed_items, typed_picks
from cpprcoder_amd import typed_split_picks as tsp
from gpu_support import Guarded, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAST = -(1 << 63)  # 2^63 as the int64 the tables hold: what entries past the count are filled with
CASES = tc.kernel_cases()
NOISE = np.random.RandomState(2424).randint(0, 256, max(int(c["lengths"].sum()) for c in CASES) + 16).astype(np.uint8)
CLASSES = [(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)]
NAMES = (None, "delta", "zigzag")


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint8))).cuda()


def scattered(lengths, rs):
    """Where each entry's bytes go: the entries take their places in a shuffled order, each start at the next residue mod 16
    with a gap of guard bytes in front of it -> (at uint64[], the size of the buffer)."""
    at = np.zeros(len(lengths), np.uint64)
    cursor = 0
    for r, k in enumerate(rs.permutation(len(lengths))):
        cursor += (r % 16 - cursor) % 16 + 16
        at[k] = cursor
        cursor += int(lengths[k])
    return at, cursor + 16


def image_with(dst, entries):
    """What the guarded buffer must hold: its pattern, and `entries` = [(at, bytes)] written into the view."""
    want = dst.before.cpu().numpy().copy()
    for at, x in entries:
        want[dst.at + int(at): dst.at + int(at) + len(x)] = x
    return want


def run_split(ctx, x, src_at, dst_at, lengths, widths, preds, count, dst, max_bytes, src_offset=0, max_pick=None, src_cap=None, dst_cap=None, kept=True):
    """One call on a guarded source and the guarded output `dst` -> (status, position), kept (numpy, or None); the source and what
    lies around the kept table are unchanged."""
    src = Guarded(max(len(x), 16), src_offset, x, salt=4)  # (a buffer of no bytes has no address: src_cap says how many are the call's)
    src_cap = len(x) if src_cap is None else src_cap
    n = len(lengths) if max_pick is None else max_pick
    d_kept = Guarded(8 * max(n, 1), 0, salt=5) if kept else None
    tsp.split_device(ctx, src.view, dev64(src_at), dev64(dst_at), dev64(lengths), dev8(widths), None if preds is None else dev8(preds), dev64([count]),
                     dst.view, max_bytes, max_pick=max_pick, kept=d_kept.view.view(torch.int64) if kept else None, src_cap=src_cap, dst_cap=dst_cap)
    st = ctx.sync_status(raise_on_error=False)
    src.check(0, "typed split picks src")
    if not kept:
        return st, None
    d_kept.check(8 * n, "typed split picks kept")
    return st, d_kept.view.view(torch.int64).cpu().numpy().astype(np.uint64)[:n]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parity(ctx, case):
    """Every batch of the typed item kernels' switch points: the items packed (every residue mod 16 on the source side through
    the batch's ragged lengths and its offset), the destinations scattered with gaps at every residue, the entries shuffled.
    Every output is split_numpy's and the host-planned call's, every other byte keeps its guard pattern, and kept is the lengths."""
    lengths, widths, preds = case["lengths"], case["widths"], case["preds"]
    n = len(lengths)
    offs = tc.offsets_of(case)
    rs = np.random.RandomState(n + 7)
    order = rs.permutation(n)
    kinds = tc.KINDS if preds.any() else ("random",)
    for kind in kinds:
        x = tc.case_bytes(case, kind, NOISE)
        y = typed_items.split_numpy(x, offs, widths, preds)
        at, size = scattered(lengths, rs)
        dst = Guarded(size, case["dst_offset"], salt=6)
        st, kept = run_split(ctx, x, offs[:-1][order], at[order], lengths[order], widths[order], preds[order], n, dst, int(lengths.sum()),
                             src_offset=case["src_offset"], max_pick=n)
        assert st[0] == rcx.OK, (kind, st)
        assert np.array_equal(kept, lengths[order]), (case["name"], kind)
        want = image_with(dst, [(at[i], y[int(offs[i]): int(offs[i + 1])]) for i in range(n)])
        assert np.array_equal(dst.tensor.cpu().numpy(), want), (case["name"], kind)
        if len(x):  # the host-planned call on the same items
            theirs = torch.zeros(len(x), dtype=torch.uint8, device="cuda")
            typed_items.split_device(ctx, dev8(x), offs, widths, preds, theirs)
            ctx.sync_status()
            assert np.array_equal(theirs.cpu().numpy(), y), (case["name"], kind)


def small_items(top):
    """`top` items of 32 bytes, the ten classes in turn -> (x, y, widths, preds): the bytes, their split text, the tables."""
    rs = np.random.RandomState(99)
    reps = 64  # (so that the content does not repeat with the classes)
    w = np.array([CLASSES[k % 10][0] for k in range(10 * reps)], np.uint8)
    p = np.array([CLASSES[k % 10][1] for k in range(10 * reps)], np.uint8)
    x = rs.randint(0, 256, 32 * len(w)).astype(np.uint8)
    offs = np.arange(len(w) + 1, dtype=np.uint64) * np.uint64(32)
    y = typed_items.split_numpy(x, offs, w, p)
    times = -(-top // len(w))
    return np.tile(x, times)[: 32 * top], np.tile(y, times)[: 32 * top], np.tile(w, times)[:top], np.tile(p, times)[:top]


def count_points():
    """Both sides of every value at which the planner's launches change shape or a loop takes another turn: a wave, a tile
    (PLAN_THREADS entries), the entry kernels' grid cap (PLAN_GRID tiles), a pass of the workgroup over the tile sums (PLAN_TOP
    tiles)."""
    edges = [64, tsp.PLAN_THREADS, tsp.PLAN_GRID * tsp.PLAN_THREADS, tsp.PLAN_TOP * tsp.PLAN_THREADS]
    return sorted({0, 1} | {m + d for m in edges for d in (-1, 0, 1)})


def test_the_count_is_read_on_the_device(ctx):
    """Items of 32 bytes of all classes; the count, under the largest max_pick, and max_pick itself on both sides of every
    planner constant.  The entries past the count hold 2^63 and are never read: nothing is latched, every meant entry is split,
    nothing else is written and kept is 0 at and behind the count.  A count above max_pick splits max_pick entries and latches
    RCX_E_CAPACITY at max_pick."""
    points = count_points()
    top = points[-1] + 5
    x, y, w, p = small_items(top)
    d_x, d_y = dev8(x), dev8(y)
    d_w, d_p = dev8(w), dev8(p)
    d_from = torch.arange(top, dtype=torch.int64, device="cuda") * 32
    d_to = d_from + 3
    d_len = torch.full((top,), 32, dtype=torch.int64, device="cuda")
    guard = Guarded(top * 32 + 3, 7, salt=8)
    kept = Guarded(8 * top, 0, salt=9)
    k64 = kept.tensor[kept.at: kept.at + 8 * top].view(torch.int64)
    index = torch.arange(top, device="cuda")
    runs = [(top, c) for c in points + [top, top + 1]] + [(m, m) for m in points[2:]] + [(points[4], points[4] + 1)]
    for max_pick, count in runs:
        live = index < count
        guard.tensor.copy_(guard.before)
        kept.tensor.copy_(kept.before)
        tsp.split_device(ctx, d_x, torch.where(live, d_from, PAST), torch.where(live, d_to, PAST), torch.where(live, d_len, PAST),
                         torch.where(live, d_w, 255).to(torch.uint8), torch.where(live, d_p, 255).to(torch.uint8), dev64([count]), guard.view,
                         32 * max_pick, max_pick=max_pick, kept=k64)
        st = ctx.sync_status(raise_on_error=False)
        meant = min(count, max_pick)
        assert st == ((rcx.OK, 0xFFFFFFFF) if count <= max_pick else (rcx.E_CAPACITY, max_pick)), (max_pick, count, st)
        want = guard.before.clone()
        want[guard.at + 3: guard.at + 3 + 32 * meant] = d_y[: 32 * meant]
        assert torch.equal(guard.tensor, want), (max_pick, count)
        kept.check(8 * max_pick, f"kept max_pick={max_pick} count={count}")
        assert torch.equal(k64[:max_pick], torch.where(index[:max_pick] < meant, 32, 0)), (max_pick, count)


@pytest.mark.parametrize("pred", [tc.NONE, tc.DELTA])
def test_pages(ctx, pred):
    """One class and one length for all entries: 1000 pages of 4096 bytes of width 2, without a predictor and with delta."""
    n, size = 1000, 4096
    x = np.random.RandomState(31 + pred).randint(0, 256, n * size).astype(np.uint8)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    w, p = np.full(n, 2, np.uint8), np.full(n, pred, np.uint8)
    y = typed_items.split_numpy(x, offs, w, p)
    slots = np.random.RandomState(5).permutation(n).astype(np.uint64) * np.uint64(size + 48) + np.uint64(5)
    dst = Guarded(n * (size + 48) + 5, 3, salt=9)
    st, kept = run_split(ctx, x, offs[:-1], slots, np.full(n, size, np.uint64), w, p if pred else None, n, dst, n * size)
    assert st[0] == rcx.OK and (kept == size).all(), st
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(slots[i], y[i * size: (i + 1) * size]) for i in range(n)]))


def test_skewed_lengths(ctx):
    """One item of 2^17 + 1 elements of width 4 with zigzag among 300 small ones of all classes: its class's rows begin and end
    inside it, the small items' classes have a few units each."""
    lengths, widths, preds, offs, x, y = good_batch()
    big = 4 * ((1 << 17) + 1) + 3
    lengths = np.concatenate([lengths[:150], [big], lengths[150:]]).astype(np.uint64)
    widths = np.concatenate([widths[:150], [4], widths[150:]]).astype(np.uint8)
    preds = np.concatenate([preds[:150], [tc.ZIGZAG], preds[150:]]).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    x = np.random.RandomState(77).randint(0, 256, int(offs[-1])).astype(np.uint8)
    x[int(offs[150]): int(offs[151]) - 3] = (np.arange((1 << 17) + 1, dtype=np.uint64) * 5).astype("<u4").view(np.uint8)
    y = typed_items.split_numpy(x, offs, widths, preds)
    at, size = scattered(lengths, np.random.RandomState(78))
    dst = Guarded(size, 5, salt=10)
    st, kept = run_split(ctx, x, offs[:-1], at, lengths, widths, preds, 301, dst, int(lengths.sum()), src_offset=9)
    assert st[0] == rcx.OK and np.array_equal(kept, lengths), st
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[i], y[int(offs[i]): int(offs[i + 1])]) for i in range(301)]))


BAD = {  # kind -> (src_at, dst_at, len, width, pred) of the bad entry, given the caps
    "width 3": lambda sc, dc: (0, 64, 100, 3, 0),
    "width 0": lambda sc, dc: (0, 64, 100, 0, 0),
    "width 16": lambda sc, dc: (0, 64, 100, 16, 0),
    "predictor 3": lambda sc, dc: (0, 64, 100, 4, 3),
    "predictor on width 1": lambda sc, dc: (0, 64, 100, 1, 1),
    "too long": lambda sc, dc: (0, 64, tsp.MAX_BLOCK + 1, 1, 0),
    "too long by its tail": lambda sc, dc: (0, 64, 8 * (tsp.MAX_BLOCK - 6) + 7, 8, 0),
    "source position past its cap": lambda sc, dc: (sc + 1, 64, 10, 2, 0),
    "source length past its cap": lambda sc, dc: (sc - 50, 64, 100, 2, 0),
    "destination position past its cap": lambda sc, dc: (0, dc + 1, 10, 2, 1),
    "destination length past its cap": lambda sc, dc: (0, dc - 50, 100, 2, 1),
    "a source that would wrap": lambda sc, dc: ((1 << 64) - 10, 64, 100, 4, 0),
    "a destination that would wrap": lambda sc, dc: (0, (1 << 64) - 10, 100, 4, 2),
}


def good_batch():
    case = next(c for c in CASES if c["name"] == "mixed small")
    lengths, widths, preds = case["lengths"][:300].copy(), case["widths"][:300].copy(), case["preds"][:300].copy()
    offs = np.zeros(301, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    x = NOISE[: int(offs[-1])].copy()
    return lengths, widths, preds, offs, x, typed_items.split_numpy(x, offs, widths, preds)


@pytest.mark.parametrize("where", [5, 200])
@pytest.mark.parametrize("kind", list(BAD))
def test_bad_entries(ctx, kind, where):
    """One bad entry among 300 good ones of all classes: status, position and kept are the model's, the good entries are split
    and nothing of the bad one is written."""
    lengths, widths, preds, offs, x, y = good_batch()
    rs = np.random.RandomState(70)
    at, size = scattered(lengths, rs)
    at += 8192  # (room for the bad entry's own destination in front)
    size += 8192
    src_at = offs[:-1].copy()
    src_at[where], at[where], lengths[where], widths[where], preds[where] = BAD[kind](len(x), size)
    model = tsp.plan_numpy(src_at, at, lengths, widths, preds, 300, len(x), len(x), size)
    want_status = rcx.E_CAPACITY if "cap" in kind or "wrap" in kind else rcx.E_CORRUPT
    assert (model["status"], model["position"]) == (want_status, where) and not model["valid"][where] and model["valid"].sum() >= 270
    assert model["kept"][where] == 0
    dst = Guarded(size, 2, salt=13)
    st, kept = run_split(ctx, x, src_at, at, lengths, widths, preds, 300, dst, len(x))
    assert st == (model["status"], where), (kind, st)
    assert np.array_equal(kept, model["kept"]), kind
    entries = [(at[k], y[int(offs[k]): int(offs[k + 1])]) for k in range(300) if model["place"][k] >= 0]
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, entries)), kind


def test_overflow_splits_nothing(ctx):
    """The valid entries' lengths at max_bytes: all are split; one byte above: nothing is written, kept is all 0 and
    RCX_E_CAPACITY is latched at the count."""
    lengths, widths, preds, offs, x, y = good_batch()
    at, size = scattered(lengths, np.random.RandomState(71))
    total = int(lengths.sum())
    for max_bytes in (total, total - 1):
        model = tsp.plan_numpy(offs[:-1], at, lengths, widths, preds, 300, max_bytes, len(x), size)
        dst = Guarded(size, 1, salt=14)
        st, kept = run_split(ctx, x, offs[:-1], at, lengths, widths, preds, 300, dst, max_bytes)
        assert np.array_equal(kept, model["kept"])
        if max_bytes == total:
            assert st[0] == rcx.OK and model["status"] == rcx.OK and np.array_equal(kept, lengths)
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], y[int(offs[k]): int(offs[k + 1])]) for k in range(300)]))
        else:
            assert model["overflow"] and st == (rcx.E_CAPACITY, 300) == (model["status"], model["position"])
            assert torch.equal(dst.tensor, dst.before) and not kept.any()


def test_without_preds_and_without_kept(ctx):
    """d_preds = NULL: no entry has a predictor; d_kept = NULL: nothing is written for it.  The output is the same call's with a
    table of zeros."""
    lengths, widths, preds, offs, x, _ = good_batch()
    y = typed_items.split_numpy(x, offs, widths, None)
    at, size = scattered(lengths, np.random.RandomState(73))
    want = None
    for with_preds, with_kept in ((False, False), (False, True), (True, False)):
        dst = Guarded(size, 6, salt=15)
        st, kept = run_split(ctx, x, offs[:-1], at, lengths, widths, np.zeros(300, np.uint8) if with_preds else None, 300, dst, len(x), kept=with_kept)
        assert st[0] == rcx.OK and (kept is None) == (not with_kept)
        if want is None:
            want = image_with(dst, [(at[k], y[int(offs[k]): int(offs[k + 1])]) for k in range(300)])
        assert np.array_equal(dst.tensor.cpu().numpy(), want), (with_preds, with_kept)
        if with_kept:
            assert np.array_equal(kept, lengths)


def test_host_buffers(ctx):
    """rcx_typed_split_picks: the same on host buffers, every entry meant.  dst comes back as a whole, so what no entry writes
    keeps its bytes; behind a latched failure the good entries are written all the same, and kept says which."""
    lengths, widths, preds, offs, x, y = good_batch()
    at, size = scattered(lengths, np.random.RandomState(72))
    pattern = ((np.arange(size) * 29 + 7) % 253 + 1).astype(np.uint8)
    dst = pattern.copy()
    st, kept = tsp.split(ctx, x, offs[:-1], at, lengths, widths, preds, dst)
    assert st == rcx.OK and np.array_equal(kept, lengths)
    want = pattern.copy()
    for k in range(300):
        want[int(at[k]): int(at[k]) + int(lengths[k])] = y[int(offs[k]): int(offs[k + 1])]
    assert np.array_equal(dst, want)
    k = next(k for k in range(300) if lengths[k] > 0)
    widths[k] = 5
    dst = pattern.copy()
    st, kept = tsp.split(ctx, x, offs[:-1], at, lengths, widths, preds, dst)
    assert st == rcx.E_CORRUPT and kept[k] == 0 and np.array_equal(np.delete(kept, k), np.delete(lengths, k))
    want[int(at[k]): int(at[k]) + int(lengths[k])] = pattern[int(at[k]): int(at[k]) + int(lengths[k])]
    assert np.array_equal(dst, want)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # (the call took the latch with it)


def test_reservations():
    """rcx_typed_split_picks_scratch_bytes is what a fresh context holds after the reservation alone; with
    rcx_typed_picks_reserve in either order the table scratch is the larger of the two; with rcx_encode_picks_reserve in either
    order it is the larger of this call's tables and the encode call's, and the encode call's other scratch stands beside it."""
    for max_pick, max_bytes, max_len in ((1000, 1 << 20, 4096), (64, 1 << 26, 70_000), (5000, 0, 100)):
        mine, join = tsp.scratch_bytes(max_pick, max_bytes), typed_picks.scratch_bytes(max_pick, max_bytes)
        assert mine == tsp.scratch_formula(max_pick, max_bytes)
        enc = encode_picks.scratch_bytes(max_pick, max_len, max_bytes)
        enc_tables = 20 * (max_pick + encode_picks.PAD) + 16 + 8 * max_pick + (2 * encode_picks.CODED_BINS + 4) * 4
        calls = {"split": lambda c: tsp.reserve(c, max_pick, max_bytes), "join": lambda c: typed_picks.reserve(c, max_pick, max_bytes),
                 "encode": lambda c: encode_picks.reserve(c, max_pick, max_len, max_bytes)}
        tables = {"split": mine, "join": join, "encode": enc_tables}
        for order in (("split", "join"), ("join", "split"), ("split", "encode"), ("encode", "split"), ("join", "encode", "split")):
            c = rcx.Context(0)
            seen = []
            for name in order:
                calls[name](c)
                seen.append(name)
                assert c.scratch_bytes() == max(tables[s] for s in seen) + (enc - enc_tables if "encode" in seen else 0), (order, name)
            c.close()


def test_round_trip_on_the_device(ctx):
    """Split picks into a packed staging buffer, join picks from it to scattered places: the items are back, both tables read
    on the device, kept the join's length table."""
    lengths, widths, preds, offs, x, y = good_batch()
    rs = np.random.RandomState(74)
    src_at, src_size = scattered(lengths, rs)
    image = np.zeros(src_size, np.uint8)
    for k in range(300):
        image[int(src_at[k]): int(src_at[k]) + int(lengths[k])] = x[int(offs[k]): int(offs[k + 1])]
    out_at, out_size = scattered(lengths, rs)
    stage = Guarded(len(x), 3, salt=19)
    out = Guarded(out_size, 4, salt=20)
    d_src_at, d_stage_at, d_out_at, d_len = dev64(src_at), dev64(offs[:-1]), dev64(out_at), dev64(lengths)
    d_w, d_p, d_count = dev8(widths), dev8(preds), dev64([300])
    d_kept = torch.zeros(300, dtype=torch.int64, device="cuda")
    tsp.split_device(ctx, dev8(image), d_src_at, d_stage_at, d_len, d_w, d_p, d_count, stage.view, len(x), kept=d_kept)
    typed_picks.join_device(ctx, stage.view, d_stage_at, d_out_at, d_kept, d_w, d_p, d_count, out.view, len(x))
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(stage.view.cpu().numpy(), y)
    stage.check(len(x), "staging")
    assert np.array_equal(out.tensor.cpu().numpy(), image_with(out, [(out_at[k], x[int(offs[k]): int(offs[k + 1])]) for k in range(300)]))


# ---- container.pack_typed_items_device -----------------------------------------------------------------------------------------
def ragged_items(seed=404, lengths=(0, 1, 7, 16, 65, 300, 1024, 1025, 3000, 5000, 2001, 33, 3, 0, 640, 129, 5, 4097, 2, 800)):
    """Items of all ten classes in turn with ragged lengths, among them 0 and lengths below the width: ramps with noise in the low
    bits, so that every coder has something to do -> (items as bytes, widths, preds)."""
    rs = np.random.RandomState(seed)
    items, widths, preds = [], [], []
    for k, n in enumerate(lengths):
        w, p = CLASSES[k % len(CLASSES)]
        ramp = (np.arange(n // w + 1, dtype=np.uint64) * 3 + rs.randint(0, 4, n // w + 1).astype(np.uint64)).astype(f"<u{w}")
        items.append(ramp.view(np.uint8)[:n].tobytes())
        widths.append(w)
        preds.append(p)
    return items, np.array(widths, np.uint8), np.array(preds, np.uint8)


def device_tables(items, widths, preds, max_items, gap=5):
    """The items with `gap` bytes between them in one device buffer, and the pack call's tables with garbage behind the count."""
    lengths = np.array([len(x) for x in items], np.uint64)
    at = (np.cumsum(lengths + np.uint64(gap)) - lengths).astype(np.uint64)
    image = np.full(int(at[-1] + lengths[-1]) + gap if len(items) else 16, 0xEE, np.uint8)
    for a, x in zip(at, items):
        image[int(a): int(a) + len(x)] = np.frombuffer(x, np.uint8)
    d_at = torch.full((max_items,), PAST, dtype=torch.int64, device="cuda")
    d_len = torch.full((max_items,), PAST, dtype=torch.int64, device="cuda")
    d_w = torch.full((max_items,), 255, dtype=torch.uint8, device="cuda")
    d_p = torch.full((max_items,), 255, dtype=torch.uint8, device="cuda")
    n = len(items)
    d_at[:n], d_len[:n], d_w[:n], d_p[:n] = dev64(at), dev64(lengths), dev8(widths), dev8(preds)
    return dev8(image), d_at, d_len, d_w, d_p, dev64([n]), lengths


@pytest.mark.parametrize("coder", [rcx.CODER_ADAPTIVE, rcx.CODER_STATIC, rcx.CODER_RANS, rcx.CODER_RANS8])
def test_the_container_is_the_host_planned_one(ctx, coder):
    """to_bytes() on a batch of all ten classes with ragged lengths is byte for byte what container.pack_typed_items writes for the
    same items, widths and predictors, and unpack_typed_items gives the items."""
    items, widths, preds = ragged_items()
    theirs = container.pack_typed_items(items, widths=[int(w) for w in widths], predict=[NAMES[int(p)] for p in preds], coder=coder, ctx=ctx)
    max_items = len(items) + 3
    d_src, d_at, d_len, d_w, d_p, d_count, lengths = device_tables(items, widths, preds, max_items)
    packed = container.pack_typed_items_device(ctx, d_src, d_at, d_len, d_w, d_p, d_count, max_items, int(lengths.max()), int(lengths.sum()), coder=coder)
    blob = packed.to_bytes()
    assert blob == theirs
    assert container.unpack_typed_items(blob, ctx=ctx) == items


def test_pick_naming(ctx):
    """An item above max_len alone latches RCX_E_CAPACITY at its pick; with an item of a bad width in front of it RCX_E_CORRUPT is
    latched at that one's pick.  Both are named through pick_of, neither moves another item's staging position, and the other items
    round-trip."""
    items, widths, preds = ragged_items(seed=405)
    n = len(items)
    lengths = np.array([len(x) for x in items], np.uint64)
    long_one, bad_width = 9, 4  # 5000 bytes; 65 bytes
    max_len = 4097
    assert lengths[long_one] > max_len and all(int(m) <= max_len for k, m in enumerate(lengths) if k != long_one)
    counted = np.where(np.arange(n) == long_one, 0, lengths).astype(np.int64)
    stage_at = np.cumsum(counted) - counted
    for break_width, want in ((False, (rcx.E_CAPACITY, long_one)), (True, (rcx.E_CORRUPT, bad_width))):
        w = widths.copy()
        if break_width:
            w[bad_width] = 3
        d_src, d_at, d_len, d_w, d_p, d_count, _ = device_tables(items, w, preds, n + 2)
        packed = container.pack_typed_items_device(ctx, d_src, d_at, d_len, d_w, d_p, d_count, n + 2, max_len, int(lengths.sum()))
        st, position = ctx.sync_status(raise_on_error=False)
        assert (st, packed.pick_of(position)) == want and position % 8 == 0, (break_width, st, position)
        assert np.array_equal(packed.stage_at.cpu().numpy()[:n], stage_at)
        lost = {long_one, bad_width} if break_width else {long_one}
        kept = packed.d_lengths.cpu().numpy()
        assert [int(x) for x in kept[:n]] == [0 if k in lost else int(lengths[k]) for k in range(n)] and not kept[n:].any()
        out_at, size = scattered(lengths, np.random.RandomState(80))
        dst = Guarded(size, 3, salt=21)
        packed.reserve(n, int(lengths.sum()))
        packed.decode_into(torch.arange(n, dtype=torch.int64, device="cuda"), dev64(out_at), dev64([n]), dst.view, n)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(out_at[k], np.frombuffer(items[k], np.uint8)) for k in range(n) if k not in lost]))


def test_graph_capture_and_replay():
    """Reserve, capture pack_typed_items_device and PackedTypedItems.decode_into once (a linear graph on one stream), replay three
    times; between the replays the items' bytes, every table of the pack call, the picks, the destinations and both counts are
    rewritten by torch ops on the device only.  Every replay's output is the items it named, and the context's scratch is what it
    was before the capture."""
    fresh = rcx.Context(0)
    try:
        pool = 40
        rs = np.random.RandomState(90)
        plen = rs.randint(0, 3000, pool).astype(np.uint64)
        plen[:3] = (0, 1, 2999)
        pw = np.array([CLASSES[k % 10][0] for k in range(pool)], np.uint8)
        pp = np.array([CLASSES[k % 10][1] for k in range(pool)], np.uint8)
        pat = (np.cumsum(plen + np.uint64(7)) - plen).astype(np.uint64)
        size = int(pat[-1] + plen[-1]) + 7
        images = [np.random.RandomState(91 + r).randint(0, 256, size).astype(np.uint8) & np.uint8(0x3F >> r) for r in range(3)]
        d_images = [dev8(x) for x in images]
        d_pat, d_plen, d_pw, d_pp = dev64(pat), dev64(plen), dev8(pw), dev8(pp)
        max_items, max_len = 32, 2999
        max_bytes = max_items * max_len
        d_src = torch.zeros(size, dtype=torch.uint8, device="cuda")
        d_at = torch.zeros(max_items, dtype=torch.int64, device="cuda")
        d_len = torch.zeros_like(d_at)
        d_w = torch.ones(max_items, dtype=torch.uint8, device="cuda")
        d_p = torch.zeros(max_items, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_pick = torch.zeros(max_items, dtype=torch.int64, device="cuda")
        d_out_at = torch.zeros_like(d_pick)
        d_npick = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = Guarded(max_items * (max_len + 40), 11, salt=12)
        S = tsp.SLOTS
        tsp.reserve(fresh, S * max_items, max_bytes)
        encode_picks.reserve(fresh, S * max_items, max_len, max_bytes)
        picks.reserve(fresh, S * max_items, max_len)
        typed_picks.reserve(fresh, S * max_items, max_bytes)
        before = fresh.scratch_bytes()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            packed = container.pack_typed_items_device(fresh, d_src, d_at, d_len, d_w, d_p, d_count, max_items, max_len, max_bytes)
            packed.decode_into(d_pick, d_out_at, d_npick, dst.view, max_items)
        assert fresh.scratch_bytes() == before
        index = torch.arange(max_items, device="cuda")
        for replay, (mul, add, count) in enumerate(((7, 3, 32), (11, 5, 10), (13, 1, 27))):
            chosen = (index * mul + add) % pool
            live = index < count
            d_src.copy_(d_images[replay])
            d_at.copy_(torch.where(live, d_pat[chosen], PAST))
            d_len.copy_(torch.where(live, d_plen[chosen], PAST))
            d_w.copy_(torch.where(live, d_pw[chosen], 255).to(torch.uint8))
            d_p.copy_(torch.where(live, d_pp[chosen], 255).to(torch.uint8))
            d_count.fill_(count)
            d_pick.copy_(torch.where(live, count - 1 - index, PAST))  # the items in reverse
            n_of_pick = d_plen[chosen][torch.clamp(count - 1 - index, 0, max_items - 1)]
            d_out_at.copy_(torch.cumsum(n_of_pick + 17 + replay, 0) - n_of_pick)
            d_npick.fill_(count)
            dst.tensor.copy_(dst.before)
            g.replay()
            torch.cuda.synchronize()
            assert fresh.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            c, a = chosen.cpu().numpy(), d_out_at.cpu().numpy()
            entries = []
            for k in range(count):
                i = int(c[count - 1 - k])
                entries.append((a[k], images[replay][int(pat[i]): int(pat[i]) + int(plen[i])]))
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, entries)), replay
            assert fresh.scratch_bytes() == before, replay
    finally:
        fresh.close()
