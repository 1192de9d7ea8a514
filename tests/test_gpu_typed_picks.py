"""rcx_typed_join_picks_device on the GPU (include/rcx_typed_picks.h): the typed join per item whose positions, lengths, widths,
predictors and count are read from device memory, planned by kernels, capturable in a graph; and container.open_typed_items
on top of it and of rcx_decode_picks_device.  Expected bytes are typed_items.join_numpy's and the host-planned call's; what is
latched is what cpprcoder_amd/typed_picks.py's numpy model of the planner says.  Every output buffer is guarded and compared
whole.  Nothing here reads the reference's tree."""
import numpy as np
import pytest

import large_cases
import typed_items_cases as tc
from cpprcoder_amd import container, rcx, typed_items, typed_picks
from gpu_support import Guarded, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAST = -(1 << 63)  # 2^63 as the int64 the tables hold: what entries past the count are filled with
CASES = tc.kernel_cases()
NOISE = np.random.RandomState(2121).randint(0, 256, max(int(c["lengths"].sum()) for c in CASES) + 16).astype(np.uint8)


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


def run_join(ctx, y, src_at, dst_at, lengths, widths, preds, count, dst, max_bytes, src_offset=0, max_pick=None, src_cap=None, dst_cap=None):
    """One call on a guarded source and the guarded output `dst` -> (status, position); the source is unchanged."""
    src = Guarded(max(len(y), 16), src_offset, y, salt=4)  # (a buffer of no bytes has no address: src_cap says how many are the call's)
    src_cap = len(y) if src_cap is None else src_cap
    typed_picks.join_device(ctx, src.view, dev64(src_at), dev64(dst_at), dev64(lengths), dev8(widths), None if preds is None else dev8(preds),
                            dev64([count]), dst.view, max_bytes, max_pick=max_pick, src_cap=src_cap, dst_cap=dst_cap)
    st = ctx.sync_status(raise_on_error=False)
    src.check(0, "typed picks src")
    return st


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parity(ctx, case):
    """Every batch of the typed item kernels' switch points: the split text packed (every residue mod 16 on the source side
    through the batch's ragged lengths and its offset), the destinations scattered with gaps at every residue, the entries
    shuffled.  Every output is join_numpy's and the host-planned call's, and every other byte keeps its guard pattern."""
    lengths, widths, preds = case["lengths"], case["widths"], case["preds"]
    n = len(lengths)
    offs = tc.offsets_of(case)
    rs = np.random.RandomState(n + 7)
    order = rs.permutation(n)
    kinds = tc.KINDS if preds.any() else ("random",)
    for kind in kinds:
        x = tc.case_bytes(case, kind, NOISE)
        y = typed_items.split_numpy(x, offs, widths, preds)
        assert np.array_equal(typed_items.join_numpy(y, offs, widths, preds), x)
        at, size = scattered(lengths, rs)
        dst = Guarded(size, case["dst_offset"], salt=6)
        st = run_join(ctx, y, offs[:-1][order], at[order], lengths[order], widths[order], preds[order], n, dst, int(lengths.sum()), src_offset=case["src_offset"],
                      max_pick=n)
        assert st[0] == rcx.OK, (kind, st)
        want = image_with(dst, [(at[i], x[int(offs[i]): int(offs[i + 1])]) for i in range(n)])
        assert np.array_equal(dst.tensor.cpu().numpy(), want), (case["name"], kind)
        if len(x):  # the host-planned call on the same items
            theirs = torch.zeros(len(x), dtype=torch.uint8, device="cuda")
            typed_items.join_device(ctx, dev8(y), offs, widths, preds, theirs)
            ctx.sync_status()
            assert np.array_equal(theirs.cpu().numpy(), x), (case["name"], kind)


def test_residues_of_parity_cover_both_sides():
    """The batches' sources and the scattered destinations stand at every residue mod 16."""
    src = {(int(o) + c["src_offset"]) % 16 for c in CASES for o, m in zip(tc.offsets_of(c)[:-1], c["lengths"]) if m}
    rs = np.random.RandomState(3)
    at, _ = scattered(CASES[0]["lengths"], rs)
    assert src == set(range(16)) and {int(a) % 16 for a in at} == set(range(16))


def small_items(top):
    """`top` items of 32 bytes, the ten classes in turn -> (x, y, widths, preds): the bytes, their split text, the tables."""
    classes = [(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)]
    rs = np.random.RandomState(99)
    reps = 64  # (so that the content does not repeat with the classes)
    w = np.array([classes[k % 10][0] for k in range(10 * reps)], np.uint8)
    p = np.array([classes[k % 10][1] for k in range(10 * reps)], np.uint8)
    x = rs.randint(0, 256, 32 * len(w)).astype(np.uint8)
    offs = np.arange(len(w) + 1, dtype=np.uint64) * np.uint64(32)
    y = typed_items.split_numpy(x, offs, w, p)
    times = -(-top // len(w))
    return np.tile(x, times)[: 32 * top], np.tile(y, times)[: 32 * top], np.tile(w, times)[:top], np.tile(p, times)[:top]


def count_points():
    """Both sides of every value at which the planner's launches change shape or a loop takes another turn: a wave, a tile
    (PLAN_THREADS entries), the entry kernels' grid cap (PLAN_GRID tiles), a pass of the workgroup over the tile sums (PLAN_TOP
    tiles)."""
    edges = [64, typed_picks.PLAN_THREADS, typed_picks.PLAN_GRID * typed_picks.PLAN_THREADS, typed_picks.PLAN_TOP * typed_picks.PLAN_THREADS]
    return sorted({0, 1} | {m + d for m in edges for d in (-1, 0, 1)})


def test_the_count_is_read_on_the_device(ctx):
    """Items of 32 bytes of all classes; the count, under the largest max_pick, and max_pick itself on both sides of every
    planner constant.  The entries past the count hold 2^63 and are never read: nothing is latched, every meant entry joins and
    nothing else is written.  A count above max_pick joins max_pick entries and latches RCX_E_CAPACITY at max_pick."""
    points = count_points()
    top = points[-1] + 5
    x, y, w, p = small_items(top)
    d_x, d_y = dev8(x), dev8(y)
    d_w, d_p = dev8(w), dev8(p)
    d_from = torch.arange(top, dtype=torch.int64, device="cuda") * 32
    d_to = d_from + 3
    d_len = torch.full((top,), 32, dtype=torch.int64, device="cuda")
    guard = Guarded(top * 32 + 3, 7, salt=8)
    index = torch.arange(top, device="cuda")
    runs = [(top, c) for c in points + [top, top + 1]] + [(m, m) for m in points[2:]] + [(points[4], points[4] + 1)]
    for max_pick, count in runs:
        live = index < count
        guard.tensor.copy_(guard.before)
        typed_picks.join_device(ctx, d_y, torch.where(live, d_from, PAST), torch.where(live, d_to, PAST), torch.where(live, d_len, PAST),
                                torch.where(live, d_w, 255).to(torch.uint8), torch.where(live, d_p, 255).to(torch.uint8), dev64([count]), guard.view,
                                32 * max_pick, max_pick=max_pick)
        st = ctx.sync_status(raise_on_error=False)
        meant = min(count, max_pick)
        assert st == ((rcx.OK, 0xFFFFFFFF) if count <= max_pick else (rcx.E_CAPACITY, max_pick)), (max_pick, count, st)
        want = guard.before.clone()
        want[guard.at + 3: guard.at + 3 + 32 * meant] = d_x[: 32 * meant]
        assert torch.equal(guard.tensor, want), (max_pick, count)


@pytest.mark.parametrize("pred", [tc.NONE, tc.DELTA])
def test_pages(ctx, pred):
    """One class and one length for all entries: 1000 pages of 4096 bytes of width 2; with delta the scan list is one bin."""
    n, size = 1000, 4096
    x = np.random.RandomState(31 + pred).randint(0, 256, n * size).astype(np.uint8)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    w, p = np.full(n, 2, np.uint8), np.full(n, pred, np.uint8)
    y = typed_items.split_numpy(x, offs, w, p)
    slots = np.random.RandomState(5).permutation(n).astype(np.uint64) * np.uint64(size + 48) + np.uint64(5)
    dst = Guarded(n * (size + 48) + 5, 3, salt=9)
    st = run_join(ctx, y, offs[:-1], slots, np.full(n, size, np.uint64), w, p if pred else None, n, dst, n * size)
    assert st[0] == rcx.OK, st
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(slots[i], x[i * size: (i + 1) * size]) for i in range(n)]))


BAD = {  # kind -> (src_at, dst_at, len, width, pred) of the bad entry, given the caps
    "width 3": lambda sc, dc: (0, 64, 100, 3, 0),
    "width 0": lambda sc, dc: (0, 64, 100, 0, 0),
    "width 16": lambda sc, dc: (0, 64, 100, 16, 0),
    "predictor 3": lambda sc, dc: (0, 64, 100, 4, 3),
    "predictor on width 1": lambda sc, dc: (0, 64, 100, 1, 1),
    "too long": lambda sc, dc: (0, 64, typed_picks.MAX_BLOCK + 1, 1, 0),
    "too long by its tail": lambda sc, dc: (0, 64, 8 * (typed_picks.MAX_BLOCK - 6) + 7, 8, 0),
    "source past its cap": lambda sc, dc: (sc - 50, 64, 100, 2, 0),
    "destination past its cap": lambda sc, dc: (0, dc - 50, 100, 2, 1),
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
    """One bad entry among 300 good ones of all classes: status and position are the model's, the good entries are joined and
    nothing of the bad one is written."""
    lengths, widths, preds, offs, x, y = good_batch()
    rs = np.random.RandomState(70)
    at, size = scattered(lengths, rs)
    at += 8192  # (room for the bad entry's own destination in front)
    size += 8192
    src_at = offs[:-1].copy()
    src_at[where], at[where], lengths[where], widths[where], preds[where] = BAD[kind](len(y), size)
    model = typed_picks.plan_numpy(src_at, at, lengths, widths, preds, 300, len(y), len(y), size)
    want_status = rcx.E_CAPACITY if "cap" in kind or "wrap" in kind else rcx.E_CORRUPT
    assert (model["status"], model["position"]) == (want_status, where) and not model["valid"][where] and model["valid"].sum() >= 270
    dst = Guarded(size, 2, salt=13)
    st = run_join(ctx, y, src_at, at, lengths, widths, preds, 300, dst, len(y))
    assert st == (model["status"], where), (kind, st)
    entries = [(at[k], x[int(offs[k]): int(offs[k + 1])]) for k in range(300) if model["route"][k]]
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, entries)), kind


def test_overflow_joins_nothing(ctx):
    """The valid entries' lengths at max_bytes: all join; one byte above: nothing is written and RCX_E_CAPACITY is latched at the count."""
    lengths, widths, preds, offs, x, y = good_batch()
    at, size = scattered(lengths, np.random.RandomState(71))
    total = int(lengths.sum())
    for max_bytes in (total, total - 1):
        model = typed_picks.plan_numpy(offs[:-1], at, lengths, widths, preds, 300, max_bytes, len(y), size)
        dst = Guarded(size, 1, salt=14)
        st = run_join(ctx, y, offs[:-1], at, lengths, widths, preds, 300, dst, max_bytes)
        if max_bytes == total:
            assert st[0] == rcx.OK and model["status"] == rcx.OK
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], x[int(offs[k]): int(offs[k + 1])]) for k in range(300)]))
        else:
            assert model["overflow"] and st == (rcx.E_CAPACITY, 300) == (model["status"], model["position"])
            assert torch.equal(dst.tensor, dst.before)


def test_past_4_gib(ctx):
    """A destination of 4 GiB + 1 MiB with entries placed behind 2^32 (and one across it): the touched windows hold the joined
    bytes, and a guard band around each keeps its fill."""
    lengths, widths, preds, offs, x, y = good_batch()
    cap = (1 << 32) + (1 << 20)
    whole, view = large_cases.guarded(cap, offset=3, guard=64, fill=0xA5)
    base = (1 << 32) - 1000  # the window: the first entries lie across 2^32, the rest behind it
    at = np.uint64(base) + offs[:-1] + np.arange(300, dtype=np.uint64) * np.uint64(3)
    window = int(at[-1] + lengths[-1]) - base
    assert base + window + 4096 <= cap
    typed_picks.join_device(ctx, dev8(y), dev64(offs[:-1]), dev64(at), dev64(lengths), dev8(widths), dev8(preds), dev64([300]), view, len(y))
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    want = np.full(window + 8192, 0xA5, np.uint8)
    for k in range(300):
        a = int(at[k]) - base + 4096
        want[a: a + int(lengths[k])] = x[int(offs[k]): int(offs[k + 1])]
    assert np.array_equal(view[base - 4096: base + window + 4096].cpu().numpy(), want)
    low = (base & 0xFFFFFFFF) if base >> 32 else 0  # where a position cut to 32 bits would have written
    assert large_cases.all_bytes(view[low: low + (1 << 20)], 0xA5) and large_cases.all_bytes(whole[:67], 0xA5) and large_cases.all_bytes(whole[-64:], 0xA5)


def test_host_buffers(ctx):
    """rcx_typed_join_picks: the same on host buffers, every entry meant.  dst comes back as a whole, so what no entry writes
    keeps its bytes; behind a latched failure the good entries are written all the same."""
    lengths, widths, preds, offs, x, y = good_batch()
    at, size = scattered(lengths, np.random.RandomState(72))
    pattern = ((np.arange(size) * 29 + 7) % 253 + 1).astype(np.uint8)
    dst = pattern.copy()
    assert typed_picks.join(ctx, y, offs[:-1], at, lengths, widths, preds, dst) == rcx.OK
    want = pattern.copy()
    for k in range(300):
        want[int(at[k]): int(at[k]) + int(lengths[k])] = x[int(offs[k]): int(offs[k + 1])]
    assert np.array_equal(dst, want)
    k = next(k for k in range(300) if lengths[k] > 0)
    widths[k] = 5
    dst = pattern.copy()
    assert typed_picks.join(ctx, y, offs[:-1], at, lengths, widths, preds, dst) == rcx.E_CORRUPT
    want[int(at[k]): int(at[k]) + int(lengths[k])] = pattern[int(at[k]): int(at[k]) + int(lengths[k])]
    assert np.array_equal(dst, want)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # (the call took the latch with it)


# ---- container.open_typed_items ------------------------------------------------------------------------------------------------
def typed_blob(ctx, made):
    """-> (blob, items): a version-1 container of mixed widths and predictors; a version-2 one with stored sub-items (bf16 randn,
    eight-state rANS: the high planes compress, the mantissa planes are stored); a checked one."""
    rs = np.random.RandomState(404)
    if made == "stored":
        items = [torch.randn(n, generator=torch.Generator().manual_seed(n)).to(torch.bfloat16).view(torch.int16).numpy().tobytes() for n in (5000, 300, 1, 0, 8193, 2000)]
        blob = container.pack_typed_items(items, widths=2, coder=rcx.CODER_RANS8, stored=True, ctx=ctx)
        c = container.parse_typed_items(blob)
        assert c.get("stored") is not None and c["stored"].any() and not c["stored"].all()
        return blob, items
    lengths = [0, 1, 7, 16, 65, 300, 1024, 1025, 3000, 5000, 20_001, 33] * 2
    classes = [(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)]
    items, widths, preds = [], [], []
    for k, n in enumerate(lengths):
        w, p = classes[k % len(classes)]
        ramp = (np.arange(n // max(w, 1) + 1, dtype=np.uint64) * 3 + rs.randint(0, 4, n // max(w, 1) + 1).astype(np.uint64)).astype(f"<u{w}")
        items.append(ramp.view(np.uint8)[:n].tobytes())
        widths.append(w)
        preds.append((None, "delta", "zigzag")[p])
    blob = container.pack_typed_items(items, widths=widths, predict=preds, ctx=ctx, checksum=made == "checked")
    return blob, items


def picks_for(box, rs, extra=7):
    pick = np.concatenate([rs.permutation(box.nitems), rs.randint(0, box.nitems, 10)])
    plen = box.lengths[pick]
    at, size = scattered(plen, rs)
    max_pick = len(pick) + extra
    d_pick = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
    d_at = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
    d_pick[: len(pick)], d_at[: len(pick)] = dev64(pick), dev64(at)
    return pick, plen, at, size, max_pick, d_pick, d_at


@pytest.mark.parametrize("made", ["plain", "stored", "checked"])
def test_open_typed_items(ctx, made):
    """A typed container opened once on the device; decode_into a scattered layout gives, entry by entry, what unpack_typed_items
    gives for the same picks, shuffled and with repeats; a pick outside the container is latched at its position."""
    blob, items = typed_blob(ctx, made)
    rs = np.random.RandomState(17)
    with container.open_typed_items(blob, ctx=ctx) as box:
        assert box.nitems == len(items)
        pick, plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs)
        want = container.unpack_typed_items(blob, pick=[int(i) for i in pick], ctx=ctx)
        assert [len(x) for x in want] == [int(n) for n in plen] and want == [items[int(i)] for i in pick]
        dst = Guarded(size, 4, salt=16)
        box.reserve(max_pick, int(plen.sum()))
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], np.frombuffer(want[k], np.uint8)) for k in range(len(pick))]))
        if made == "checked":
            box.verify(pick)
        k = next(k for k in range(len(pick)) if plen[k])
        d_pick[k] = len(items)
        dst.tensor.copy_(dst.before)
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        st, position = ctx.sync_status(raise_on_error=False)
        assert st == rcx.E_CORRUPT and box.pick_of(position) == k
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[j], np.frombuffer(want[j], np.uint8)) for j in range(len(pick)) if j != k]))


def test_open_typed_items_damage(ctx):
    """A checked container with one payload bit flipped in a stream that still decodes: verify raises ChecksumError with the item's
    number.  A truncated stream is latched at its pick."""
    blob, items = typed_blob(ctx, "checked")
    c = container.parse_typed_items(blob)
    head = len(blob) - len(c["payload"])
    victim = 9  # 5000 bytes
    sub = int(c["sub_first"][victim])
    a, b = int(c["offsets"][sub]), int(c["offsets"][sub + 1])
    rs = np.random.RandomState(18)
    found = None
    for back in (5, 6, 7, 8, 10, 12, 16, 24, 32, (b - a) // 2):  # the first flip whose stream still decodes, and to other bytes
        flipped = bytearray(blob)
        flipped[head + b - back] ^= 0x10
        with container.open_typed_items(bytes(flipped), ctx=ctx) as box:
            pick, plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs)
            dst = Guarded(size, 4, salt=17)
            box.reserve(max_pick, int(plen.sum()))
            box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
            st, position = ctx.sync_status(raise_on_error=False)
            if st != rcx.OK:  # the decoder saw it itself: latched at a pick of the item
                assert st == rcx.E_CORRUPT and pick[box.pick_of(position)] == victim, (back, st, position)
                continue
            try:
                box.verify(pick)
            except container.ChecksumError as e:  # the stream still decodes: only the checksums see it
                assert e.index == victim and f"item {victim}" in str(e), str(e)
                found = back
                break
    assert found is not None, "no flipped bit left a stream that decodes to other bytes"
    # the stream cut short by 40 bytes, the streams behind it moved up
    assert b - a > 80
    offsets = np.array(c["offsets"], dtype=np.uint64)
    offsets[sub + 1:] -= np.uint64(40)
    short = dict(c, crcs=None, offsets=offsets, payload=np.concatenate([c["payload"][: b - 40], c["payload"][b:]]))
    with container.OpenTypedItems(short, ctx) as box:
        pick, plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs)
        dst = Guarded(size, 4, salt=18)
        box.reserve(max_pick, int(plen.sum()))
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        st, position = ctx.sync_status(raise_on_error=False)
        assert st == rcx.E_CORRUPT and pick[box.pick_of(position)] == victim, (st, position)
        for k, i in enumerate(pick):  # every other pick is joined
            if int(i) != victim:
                assert dst.view[int(at[k]): int(at[k]) + int(plen[k])].cpu().numpy().tobytes() == items[int(i)], k


def test_reservations():
    """rcx_typed_picks_scratch_bytes is what a fresh context holds after the reservation alone; with rcx_picks_reserve in either
    order the table scratch is the larger of the two and the decode call's redo marks stand beside it."""
    from cpprcoder_amd import picks
    for max_pick, max_bytes, max_len in ((1000, 1 << 20, 4096), (64, 1 << 26, 70_000), (5000, 0, 100)):
        typed = typed_picks.scratch_bytes(max_pick, max_bytes)
        redo = (max_pick + 1) * 4
        decode = picks.scratch_bytes(max_pick, max_len) - redo  # its tables
        c = rcx.Context(0)
        typed_picks.reserve(c, max_pick, max_bytes)
        assert c.scratch_bytes() == typed == typed_picks.scratch_formula(max_pick, max_bytes)
        picks.reserve(c, max_pick, max_len)
        first = c.scratch_bytes()
        c.close()
        c = rcx.Context(0)
        picks.reserve(c, max_pick, max_len)
        assert c.scratch_bytes() == decode + redo
        typed_picks.reserve(c, max_pick, max_bytes)
        assert c.scratch_bytes() == first == max(typed, decode) + redo
        c.close()


def test_graph_capture_and_replay():
    """Reserve, capture decode_into once (a linear graph on one stream), replay three times; between the replays the picks, the
    destinations and the count are rewritten by torch ops on the device only.  Every replay's output is unpack_typed_items of its
    picks, and the context's scratch is what it was before the capture: the two calls' reservations combined."""
    c = rcx.Context(0)
    try:
        blob, items = typed_blob(c, "plain")
        n, max_pick = len(items), 96
        want = [np.frombuffer(x, np.uint8) for x in container.unpack_typed_items(blob, ctx=c)]
        longest = max(len(x) for x in items)
        max_bytes = max_pick * longest
        fresh = rcx.Context(0)
        box = container.open_typed_items(blob, ctx=fresh)
        box.reserve(max_pick, max_bytes)
        before = fresh.scratch_bytes()
        from cpprcoder_amd import picks
        decode = picks.scratch_bytes(8 * max_pick, box.max_sub_len, box.coder)
        redo = (8 * max_pick + 1) * 4
        assert before == max(decode - redo, typed_picks.scratch_bytes(8 * max_pick, max_bytes)) + redo
        assert typed_picks.scratch_bytes(8 * max_pick, max_bytes) == typed_picks.scratch_formula(8 * max_pick, max_bytes)
        d_lengths = dev64(box.lengths)
        d_pick = torch.zeros(max_pick, dtype=torch.int64, device="cuda")
        d_at = torch.zeros_like(d_pick)
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        size = max_pick * (longest + 32)
        dst = Guarded(size, 11, salt=12)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            box.decode_into(d_pick, d_at, d_count, dst.view, max_pick)
        for replay, (mul, add, count) in enumerate(((7, 3, 96), (11, 5, 10), (13, 1, 65))):
            d_pick.copy_((torch.arange(max_pick, device="cuda") * mul + add) % n)
            d_len = d_lengths[d_pick]
            d_at.copy_(torch.cumsum(d_len + 17 + replay, 0) - d_len)
            d_count.fill_(count)
            dst.tensor.copy_(dst.before)
            g.replay()
            torch.cuda.synchronize()
            assert fresh.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            p, a = d_pick.cpu().numpy(), d_at.cpu().numpy()
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(a[k], want[int(p[k])]) for k in range(count)])), replay
        assert fresh.scratch_bytes() == before
        box.close()
        fresh.close()
    finally:
        c.close()
