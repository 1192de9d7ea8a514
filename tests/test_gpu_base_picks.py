"""rcx_base_join_picks_device on the GPU (include/rcx_base_picks.h): the join per item against base spans whose positions,
lengths, widths, predictors, ops and count are read from device memory, planned by kernels, capturable in a graph; and
container.open_delta_items on top of it and of rcx_decode_picks_device.  Expected bytes are base_items.join_numpy's and the
host-planned call's; what is latched is what cpprcoder_amd/base_picks.py's numpy model of the planner says.  Every output
buffer is guarded and compared whole.  Nothing here reads the reference's tree."""
import numpy as np
import pytest

import base_items_cases as bc
import base_picks_cases as pc
import large_cases
from cpprcoder_amd import base_items, base_picks, container, picks, rcx, typed_picks
from gpu_support import Guarded, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAST = -(1 << 63)  # 2^63 as the int64 the tables hold: what entries past the count are filled with
NB = base_items.NO_BASE
CASES = bc.kernel_cases()
NOISE = np.random.RandomState(2222).randint(0, 256, 2 * max(int(c["lengths"].sum()) for c in CASES) + 64).astype(np.uint8)


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint8))).cuda()


def image_with(dst, entries):
    """What the guarded buffer must hold: its pattern, and `entries` = [(at, bytes)] written into the view."""
    want = dst.before.cpu().numpy().copy()
    for at, x in entries:
        want[dst.at + int(at): dst.at + int(at) + len(x)] = x
    return want


def run_join(ctx, y, ref, src_at, base_at, dst_at, lengths, widths, preds, ops, count, dst, max_bytes, src_offset=0, base_offset=0, max_pick=None):
    """One call on a guarded source, a guarded base and the guarded output `dst` -> (status, position); source and base are unchanged."""
    src = Guarded(max(len(y), 16), src_offset, y, salt=4)  # (a buffer of no bytes has no address: the caps say how many are the call's)
    base = Guarded(max(len(ref), 16), base_offset, ref, salt=5)
    base_picks.join_device(ctx, src.view, base.view, dev64(src_at), dev64(base_at), dev64(dst_at), dev64(lengths), dev8(widths),
                           None if preds is None else dev8(preds), dev8(ops), dev64([count]), dst.view, max_bytes, max_pick=max_pick, src_cap=len(y),
                           base_cap=len(ref))
    st = ctx.sync_status(raise_on_error=False)
    src.check(0, "base picks src")
    base.check(0, "base picks base")
    return st


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parity(ctx, case):
    """Every batch of the base item kernels' switch points: the split text packed at the batch's source offset, the base at its
    base offset, the destinations scattered with gaps at every residue, the entries shuffled; an entry without an op has a base
    offset far outside.  Every output is join_numpy's and the host-planned call's, and every other byte keeps its guard pattern."""
    lengths, widths, preds, ops = case["lengths"], case["widths"], case["preds"], case["ops"]
    n = len(lengths)
    t = pc.parity_tables(case)
    offs, boffs, at, order = t["offs"], t["boffs"], t["at"], t["order"]
    for kind in (bc.KINDS if (ops != NB).any() else ("random",)):
        x, ref = bc.case_data(case, kind, NOISE)
        y = base_items.split_numpy(x, ref, offs, boffs, widths, preds, ops)
        assert np.array_equal(base_items.join_numpy(y, ref, offs, boffs, widths, preds, ops), x)
        dst = Guarded(t["size"], case["dst_offset"], salt=6)
        st = run_join(ctx, y, ref, offs[:-1][order], boffs[order], at[order], lengths[order], widths[order], preds[order], ops[order], n, dst,
                      int(lengths.sum()), src_offset=case["src_offset"], base_offset=case["base_offset"], max_pick=n)
        assert st[0] == rcx.OK, (kind, st)
        want = image_with(dst, [(at[i], x[int(offs[i]): int(offs[i + 1])]) for i in range(n)])
        assert np.array_equal(dst.tensor.cpu().numpy(), want), (case["name"], kind)
        if len(x):  # the host-planned call on the same items
            theirs = torch.zeros(len(x), dtype=torch.uint8, device="cuda")
            base_items.join_device(ctx, dev8(y), dev8(ref) if len(ref) else None, offs, boffs, widths, preds, ops, theirs)
            ctx.sync_status()
            assert np.array_equal(theirs.cpu().numpy(), x), (case["name"], kind)


def typed_batch():
    import typed_items_cases as tc
    from cpprcoder_amd import typed_items
    case = next(c for c in tc.kernel_cases() if c["name"] == "mixed small")
    lengths, widths, preds = case["lengths"][:300].copy(), case["widths"][:300].copy(), case["preds"][:300].copy()
    offs = np.zeros(301, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    x = NOISE[: int(offs[-1])].copy()
    return lengths, widths, preds, offs, typed_items.split_numpy(x, offs, widths, preds)


def test_without_ops_it_is_the_typed_call(ctx):
    """d_ops = None: the same tables -- good entries, a corrupt one, one past its cap, a count above max_pick -- through
    typed_picks.join_device and through the new call give equal buffers and an equal latch."""
    lengths, widths, preds, offs, y = typed_batch()
    at, size = pc.scattered(lengths, np.random.RandomState(73))
    src_at = offs[:-1].copy()
    for bad, count in ((None, 300), ("width", 300), ("cap", 300), (None, 301)):
        w, a = widths.copy(), at.copy()
        if bad == "width":
            w[next(k for k in range(7, 300) if lengths[k])] = 3
        if bad == "cap":
            a[next(k for k in range(200, 300) if lengths[k])] = size - 1
        tables = (dev64(src_at), dev64(a), dev64(lengths), dev8(w), dev8(preds), dev64([count]))
        outs, latches = [], []
        for call in ("typed", "base"):
            dst = Guarded(size, 5, salt=20)
            if call == "typed":
                typed_picks.join_device(ctx, dev8(y), *tables, dst.view, len(y))
            else:
                base_picks.join_device(ctx, dev8(y), None, tables[0], None, *tables[1:5], None, tables[5], dst.view, len(y))
            latches.append(ctx.sync_status(raise_on_error=False))
            outs.append(dst.tensor.clone())
        assert latches[0] == latches[1] and torch.equal(outs[0], outs[1]), (bad, count, latches)
        assert latches[0][0] == (rcx.OK if bad is None and count == 300 else rcx.E_CORRUPT if bad == "width" else rcx.E_CAPACITY)


def small_items(top):
    """`top` items of 32 bytes, every kind of item in turn, each with a base span of its own -> (x, y, ref, widths, preds, ops)."""
    kinds = bc.ITEM_KINDS
    rs = np.random.RandomState(98)
    reps = 64  # (so that the content does not repeat with the kinds)
    w, p, o = (np.array([kinds[k % len(kinds)][j] for k in range(len(kinds) * reps)], np.uint8) for j in range(3))
    x, ref = (rs.randint(0, 256, 32 * len(w)).astype(np.uint8) for _ in range(2))
    offs = np.arange(len(w) + 1, dtype=np.uint64) * np.uint64(32)
    y = base_items.split_numpy(x, ref, offs, offs[:-1], w, p, o)
    times = -(-top // len(w))
    return tuple(np.tile(a, times)[: 32 * top] for a in (x, y, ref)) + tuple(np.tile(a, times)[:top] for a in (w, p, o))


def count_points():
    """Both sides of every value at which the planner's launches change shape or a loop takes another turn: a wave, a tile, the
    entry kernels' grid cap, a pass of the workgroup over the tile sums."""
    edges = [64, typed_picks.PLAN_THREADS, typed_picks.PLAN_GRID * typed_picks.PLAN_THREADS, typed_picks.PLAN_TOP * typed_picks.PLAN_THREADS]
    return sorted({0, 1} | {m + d for m in edges for d in (-1, 0, 1)})


def test_the_count_is_read_on_the_device(ctx):
    """Items of 32 bytes of all kinds in turn; the count, under the largest max_pick, and max_pick itself on both sides of every
    planner constant.  The entries past the count hold 2^63 and are never read: nothing is latched, every meant entry joins and
    nothing else is written.  A count above max_pick joins max_pick entries and latches RCX_E_CAPACITY at max_pick."""
    points = count_points()
    top = points[-1] + 5
    x, y, ref, w, p, o = small_items(top)
    d_x, d_y, d_ref = dev8(x), dev8(y), dev8(ref)
    d_w, d_p, d_o = dev8(w), dev8(p), dev8(o)
    d_from = torch.arange(top, dtype=torch.int64, device="cuda") * 32
    d_to = d_from + 3
    d_len = torch.full((top,), 32, dtype=torch.int64, device="cuda")
    guard = Guarded(top * 32 + 3, 7, salt=8)
    index = torch.arange(top, device="cuda")
    runs = [(top, c) for c in points + [top, top + 1]] + [(m, m) for m in points[2:]] + [(points[4], points[4] + 1)]
    for max_pick, count in runs:
        live = index < count
        guard.tensor.copy_(guard.before)
        base_picks.join_device(ctx, d_y, d_ref, torch.where(live, d_from, PAST), torch.where(live, d_from, PAST), torch.where(live, d_to, PAST),
                               torch.where(live, d_len, PAST), torch.where(live, d_w, 255).to(torch.uint8), torch.where(live, d_p, 255).to(torch.uint8),
                               torch.where(live, d_o, 77).to(torch.uint8), dev64([count]), guard.view, 32 * max_pick, max_pick=max_pick)
        st = ctx.sync_status(raise_on_error=False)
        meant = min(count, max_pick)
        assert st == ((rcx.OK, 0xFFFFFFFF) if count <= max_pick else (rcx.E_CAPACITY, max_pick)), (max_pick, count, st)
        want = guard.before.clone()
        want[guard.at + 3: guard.at + 3 + 32 * meant] = d_x[: 32 * meant]
        assert torch.equal(guard.tensor, want), (max_pick, count)


@pytest.mark.parametrize("spans", ["one", "own", "overlapping"])
@pytest.mark.parametrize("width,op", [(2, base_items.SUBZZ), (4, base_items.XOR)])
def test_pages(ctx, width, op, spans):
    """1000 pages of 4096 bytes, one class: against ONE base span, each against a span of its own, against spans that overlap."""
    n, size = 1000, 4096
    rs = np.random.RandomState(31 + width)
    x = rs.randint(0, 256, n * size).astype(np.uint8)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    stride = {"one": 0, "own": size, "overlapping": 72}[spans]
    boffs = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(5)
    ref = rs.randint(0, 256, 5 + stride * (n - 1) + size).astype(np.uint8)
    w, o = np.full(n, width, np.uint8), np.full(n, op, np.uint8)
    y = base_items.split_numpy(x, ref, offs, boffs, w, None, o)
    slots = np.random.RandomState(5).permutation(n).astype(np.uint64) * np.uint64(size + 48) + np.uint64(5)
    dst = Guarded(n * (size + 48) + 5, 3, salt=9)
    st = run_join(ctx, y, ref, offs[:-1], boffs, slots, np.full(n, size, np.uint64), w, None, o, n, dst, n * size, base_offset=1)
    assert st[0] == rcx.OK, st
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(slots[i], x[i * size: (i + 1) * size]) for i in range(n)]))


BAD = {  # kind -> (src_at, base_at, dst_at, len, width, pred, op) of the bad entry, given the caps
    "width 3": lambda sc, bc_, dc: (0, 0, 64, 100, 3, 0, 1),
    "width 0": lambda sc, bc_, dc: (0, 0, 64, 100, 0, 0, NB),
    "predictor 3": lambda sc, bc_, dc: (0, 0, 64, 100, 4, 3, NB),
    "predictor on width 1": lambda sc, bc_, dc: (0, 0, 64, 100, 1, 1, NB),
    "op 3": lambda sc, bc_, dc: (0, 0, 64, 100, 4, 0, 3),
    "op 254": lambda sc, bc_, dc: (0, 0, 64, 100, 2, 0, 254),
    "op with predictor": lambda sc, bc_, dc: (0, 0, 64, 100, 4, 1, 2),
    "too long": lambda sc, bc_, dc: (0, 0, 64, base_picks.MAX_BLOCK + 1, 1, 0, 0),
    "too long by its tail": lambda sc, bc_, dc: (0, 0, 64, 8 * (base_picks.MAX_BLOCK - 6) + 7, 8, 0, 2),
    "source past its cap": lambda sc, bc_, dc: (sc - 50, 0, 64, 100, 2, 0, 1),
    "destination past its cap": lambda sc, bc_, dc: (0, 0, dc - 50, 100, 2, 1, NB),
    "base span past its cap by one byte": lambda sc, bc_, dc: (0, bc_ - 99, 64, 100, 4, 0, 0),
    "a base span that would wrap": lambda sc, bc_, dc: (0, (1 << 64) - 10, 64, 100, 4, 0, 2),
    "a source that would wrap": lambda sc, bc_, dc: ((1 << 64) - 10, 0, 64, 100, 4, 0, NB),
}


def good_batch():
    case = next(c for c in CASES if c["name"] == "mixed small")
    case = {k: (v[:300].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    offs = bc.offsets_of(case)
    boffs, nbase = bc.base_layout(case)
    x, ref = bc.case_data(case, "random", NOISE)
    lengths, widths, preds, ops = case["lengths"], case["widths"], case["preds"], case["ops"]
    return lengths, widths, preds, ops, offs, boffs, x, ref, base_items.split_numpy(x, ref, offs, boffs, widths, preds, ops)


@pytest.mark.parametrize("where", [5, 200])
@pytest.mark.parametrize("kind", list(BAD))
def test_bad_entries(ctx, kind, where):
    """One bad entry among 300 good ones of all kinds: status and position are the model's, the good entries are joined and
    nothing of the bad one is written."""
    lengths, widths, preds, ops, offs, boffs, x, ref, y = good_batch()
    at, size = pc.scattered(lengths, np.random.RandomState(70))
    at += 8192  # (room for the bad entry's own destination in front)
    size += 8192
    src_at = offs[:-1].copy()
    src_at[where], boffs[where], at[where], lengths[where], widths[where], preds[where], ops[where] = BAD[kind](len(y), len(ref), size)
    model = base_picks.plan_numpy(src_at, boffs, at, lengths, widths, preds, ops, 300, len(y), len(y), len(ref), size)
    want_status = rcx.E_CAPACITY if "cap" in kind or "wrap" in kind else rcx.E_CORRUPT
    assert (model["status"], model["position"]) == (want_status, where) and not model["valid"][where] and model["valid"].sum() >= 270
    dst = Guarded(size, 2, salt=13)
    st = run_join(ctx, y, ref, src_at, boffs, at, lengths, widths, preds, ops, 300, dst, len(y))
    assert st == (model["status"], where), (kind, st)
    entries = [(at[k], x[int(offs[k]): int(offs[k + 1])]) for k in range(300) if model["route"][k]]
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, entries)), kind


def test_overflow_joins_nothing(ctx):
    """The valid entries' lengths at max_bytes: all join; one byte above: nothing is written and RCX_E_CAPACITY is latched at the count."""
    lengths, widths, preds, ops, offs, boffs, x, ref, y = good_batch()
    at, size = pc.scattered(lengths, np.random.RandomState(71))
    total = int(lengths.sum())
    for max_bytes in (total, total - 1):
        model = base_picks.plan_numpy(offs[:-1], boffs, at, lengths, widths, preds, ops, 300, max_bytes, len(y), len(ref), size)
        dst = Guarded(size, 1, salt=14)
        st = run_join(ctx, y, ref, offs[:-1], boffs, at, lengths, widths, preds, ops, 300, dst, max_bytes)
        if max_bytes == total:
            assert st[0] == rcx.OK and model["status"] == rcx.OK
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], x[int(offs[k]): int(offs[k + 1])]) for k in range(300)]))
        else:
            assert model["overflow"] and st == (rcx.E_CAPACITY, 300) == (model["status"], model["position"])
            assert torch.equal(dst.tensor, dst.before)


def test_past_4_gib(ctx):
    """A base and a destination of 4 GiB + 1 MiB each, allocated and not filled, with the spans in use behind 2^32 (the first
    across it): the touched window of the destination holds the joined bytes, a band around it keeps its fill, and so does the
    place where a position cut to 32 bits would have written."""
    lengths, widths, preds, ops, offs, boffs, x, ref, y = good_batch()
    cap = (1 << 32) + (1 << 20)
    d_base = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    start = (1 << 32) - 1000  # the first entries lie across 2^32, the rest behind it
    at = np.uint64(start) + offs[:-1] + np.arange(300, dtype=np.uint64) * np.uint64(3)
    window = int(at[-1] + lengths[-1]) - start
    base_at = boffs.copy()
    base_at[ops != NB] += np.uint64(start)
    assert start + max(window, len(ref)) + 4096 <= cap
    d_base[start: start + len(ref)] = dev8(ref)
    d_dst[start - 4096: start + window + 4096] = 0xA5
    d_dst[: 1 << 20] = 0xA5  # (where a position cut to 32 bits would write)
    d_base[: 1 << 20] = 0x5A
    base_picks.join_device(ctx, dev8(y), d_base, dev64(offs[:-1]), dev64(base_at), dev64(at), dev64(lengths), dev8(widths), dev8(preds), dev8(ops), dev64([300]),
                           d_dst, len(y))
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    want = np.full(window + 8192, 0xA5, np.uint8)
    for k in range(300):
        a = int(at[k]) - start + 4096
        want[a: a + int(lengths[k])] = x[int(offs[k]): int(offs[k + 1])]
    assert np.array_equal(d_dst[start - 4096: start + window + 4096].cpu().numpy(), want)
    assert large_cases.all_bytes(d_dst[: 1 << 20], 0xA5) and large_cases.all_bytes(d_base[: 1 << 20], 0x5A)
    assert np.array_equal(d_base[start: start + len(ref)].cpu().numpy(), ref)


def test_host_buffers(ctx):
    """rcx_base_join_picks: the same on host buffers, every entry meant.  dst comes back as a whole, so what no entry writes
    keeps its bytes; behind a latched failure the good entries are written all the same."""
    lengths, widths, preds, ops, offs, boffs, x, ref, y = good_batch()
    at, size = pc.scattered(lengths, np.random.RandomState(72))
    pattern = ((np.arange(size) * 29 + 7) % 253 + 1).astype(np.uint8)
    dst = pattern.copy()
    assert base_picks.join(ctx, y, ref, offs[:-1], boffs, at, lengths, widths, preds, ops, dst) == rcx.OK
    want = pattern.copy()
    for k in range(300):
        want[int(at[k]): int(at[k]) + int(lengths[k])] = x[int(offs[k]): int(offs[k + 1])]
    assert np.array_equal(dst, want)
    k = next(k for k in range(300) if lengths[k] > 0 and ops[k] != NB)
    ops[k] = 3
    dst = pattern.copy()
    assert base_picks.join(ctx, y, ref, offs[:-1], boffs, at, lengths, widths, preds, ops, dst) == rcx.E_CORRUPT
    want[int(at[k]): int(at[k]) + int(lengths[k])] = pattern[int(at[k]): int(at[k]) + int(lengths[k])]
    assert np.array_equal(dst, want)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # (the call took the latch with it)


def test_reservations():
    """rcx_base_picks_scratch_bytes is what a fresh context holds after the reservation alone; with rcx_typed_picks_reserve and
    rcx_picks_reserve in several orders the table scratch is the largest of the three and the decode call's redo marks stand
    beside it."""
    for max_pick, max_bytes, max_len in ((1000, 1 << 20, 4096), (64, 1 << 26, 70_000), (5000, 0, 100)):
        sizes = {"base": base_picks.scratch_bytes(max_pick, max_bytes), "typed": typed_picks.scratch_bytes(max_pick, max_bytes)}
        redo = (max_pick + 1) * 4
        sizes["decode"] = picks.scratch_bytes(max_pick, max_len) - redo  # its tables
        assert sizes["base"] == base_picks.scratch_formula(max_pick, max_bytes)
        calls = {"base": lambda c: base_picks.reserve(c, max_pick, max_bytes), "typed": lambda c: typed_picks.reserve(c, max_pick, max_bytes),
                 "decode": lambda c: picks.reserve(c, max_pick, max_len)}
        c = rcx.Context(0)
        calls["base"](c)
        assert c.scratch_bytes() == sizes["base"]
        c.close()
        for order in (("base", "typed", "decode"), ("decode", "base", "typed"), ("typed", "decode", "base"), ("decode", "typed", "base")):
            c = rcx.Context(0)
            seen = []
            for name in order:
                calls[name](c)
                seen.append(name)
                assert c.scratch_bytes() == max(sizes[s] for s in seen) + (redo if "decode" in seen else 0), (order, name)
            c.close()


def test_graph_capture_and_replay():
    """Reserve, capture the call once (a chain of kernel nodes on one stream), replay three times; between the replays the
    picks -- source, base and destination positions, lengths, widths, predictors -- the ops, the base offsets and the count are
    rewritten by torch ops on the device only.  Every replay's output is join_numpy's for its tables, compared whole, and the
    context's scratch is what the reservation made it."""
    kinds = bc.ITEM_KINDS
    n, max_pick = 4 * len(kinds), 96
    rs = np.random.RandomState(404)
    w, p, o = (np.array([kinds[k % len(kinds)][j] for k in range(n)], np.uint8) for j in range(3))
    lengths = rs.randint(1, 700, n).astype(np.uint64)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    y = rs.randint(0, 256, int(offs[-1])).astype(np.uint8)  # any bytes are a split text
    ref = rs.randint(0, 256, int(offs[-1]) + 64).astype(np.uint8)
    c = rcx.Context(0)
    try:
        max_bytes = max_pick * 700
        base_picks.reserve(c, max_pick, max_bytes)
        before = c.scratch_bytes()
        assert before == base_picks.scratch_bytes(max_pick, max_bytes)
        d_y, d_ref = dev8(y), dev8(ref)
        all_at, all_len, all_w, all_p, all_o = dev64(offs[:-1]), dev64(lengths), dev8(w), dev8(p), dev8(o)
        t = {name: torch.zeros(max_pick, dtype=torch.int64, device="cuda") for name in ("src_at", "base_at", "dst_at", "len")}
        t8 = {name: torch.zeros(max_pick, dtype=torch.uint8, device="cuda") for name in ("w", "p", "o")}
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = Guarded(max_pick * (700 + 32), 11, salt=12)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            base_picks.join_device(c, d_y, d_ref, t["src_at"], t["base_at"], t["dst_at"], t["len"], t8["w"], t8["p"], t8["o"], d_count, dst.view, max_bytes,
                                   max_pick=max_pick)
        for replay, (mul, add, count) in enumerate(((7, 3, 96), (11, 5, 10), (13, 1, 65))):
            index = (torch.arange(max_pick, device="cuda") * mul + add) % n
            t["src_at"].copy_(all_at[index])
            t["len"].copy_(all_len[index])
            t["base_at"].copy_(all_at[index] + 7 * replay)
            t["dst_at"].copy_(torch.cumsum(t["len"] + 17 + replay, 0) - t["len"])
            t8["w"].copy_(all_w[index])
            t8["p"].copy_(all_p[index])
            t8["o"].copy_(torch.where(all_o[index] == NB, all_o[index], (all_o[index] + replay) % 3))
            d_count.fill_(count)
            dst.tensor.copy_(dst.before)
            g.replay()
            torch.cuda.synchronize()
            assert c.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            ops = np.where(o == NB, o, (o + replay) % 3).astype(np.uint8)
            x = base_items.join_numpy(y, ref, offs, offs[:-1] + np.uint64(7 * replay), w, p, ops)
            i, a = index.cpu().numpy(), t["dst_at"].cpu().numpy()
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(a[k], x[int(offs[i[k]]): int(offs[i[k] + 1])]) for k in range(count)])), replay
        assert c.scratch_bytes() == before
    finally:
        c.close()


# ---- container.open_delta_items ------------------------------------------------------------------------------------------------
def state_dict_items(block=4096):
    """The crafted state dict as the items pack_delta_items takes -> (items, bases: one object per item or None, widths, ops, predict)."""
    named, base, predict = bc.state_dicts()
    t = bc.tensor_items(named, base, block, predict=predict)
    offs = np.zeros(len(t["lengths"]) + 1, np.uint64)
    np.cumsum(t["lengths"], out=offs[1:])
    items = [t["x"][int(offs[k]): int(offs[k + 1])].tobytes() for k in range(len(t["lengths"]))]
    bases = [t["ref"][int(b): int(b) + int(n)].tobytes() if op != NB else None for b, n, op in zip(t["base_offsets"], t["lengths"], t["ops"])]
    ops = ["subzz" if op != NB else None for op in t["ops"]]
    preds = [(None, "delta", "zigzag")[p] for p in t["preds"]]
    return items, bases, [int(w) for w in t["widths"]], ops, preds


def picks_for(box, rs, pick, extra=7):
    plen = box.lengths[pick]
    at, size = pc.scattered(plen, rs)
    max_pick = len(pick) + extra
    d_pick = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
    d_at = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
    d_pick[: len(pick)], d_at[: len(pick)] = dev64(pick), dev64(at)
    return plen, at, size, max_pick, d_pick, d_at


@pytest.fixture(scope="module")
def state():
    return state_dict_items()


@pytest.mark.parametrize("made", ["plain", "stored", "checked"])
def test_open_delta_items(ctx, state, made):
    """The crafted state dict against the one before it, packed as RCXK, opened once on the device with its bases; decode_into a
    scattered layout gives, entry by entry, what unpack_delta_items gives for the same picks: all of them shuffled, then a
    subset with repeats.  A pick outside the container is latched at its pick."""
    items, bases, widths, ops, preds = state
    blob = container.pack_delta_items(items, bases, widths=widths, ops=ops, predict=preds, ctx=ctx, stored=True if made == "stored" else None,
                                      checksum=made == "checked")
    rs = np.random.RandomState(19)
    d_bases = [None if b is None else (dev8(np.frombuffer(b, np.uint8).copy()) if k % 2 else b) for k, b in enumerate(bases)]  # (every second one lies on the device)
    with container.open_delta_items(blob, d_bases, ctx=ctx) as box:
        assert box.nitems == len(items) and box.base_cap == sum(len(b) for b in bases if b is not None)
        for pick in (rs.permutation(box.nitems), rs.randint(0, box.nitems, 40)):
            want = container.unpack_delta_items(blob, bases, pick=[int(i) for i in pick], ctx=ctx)
            assert want == [items[int(i)] for i in pick]
            plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs, pick)
            dst = Guarded(size, 4, salt=16)
            box.reserve(max_pick, int(plen.sum()))
            box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
            assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], np.frombuffer(want[k], np.uint8)) for k in range(len(pick))]))
            if made == "checked":
                box.verify(pick)
        k = 3
        d_pick[k] = len(items)
        dst.tensor.copy_(dst.before)
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        st, position = ctx.sync_status(raise_on_error=False)
        assert st == rcx.E_CORRUPT and box.pick_of(position) == k
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[j], np.frombuffer(want[j], np.uint8)) for j in range(len(pick)) if j != k]))


def test_open_delta_items_bases(ctx, state):
    """A wrong base raises BaseItemMismatchError at open, naming the item (verify=False opens it); a base given as None is
    latched RCX_E_CAPACITY at the pick of its item while the other picks decode; one object for many items is one span."""
    items, bases, widths, ops, preds = state
    blob = container.pack_delta_items(items, bases, widths=widths, ops=ops, predict=preds, ctx=ctx)
    based = [k for k, b in enumerate(bases) if b is not None]
    victim = based[5]
    wrong = list(bases)
    wrong[victim] = bytes(len(bases[victim]))
    with pytest.raises(container.BaseItemMismatchError) as e:
        container.open_delta_items(blob, wrong, ctx=ctx)
    assert e.value.index == victim
    container.open_delta_items(blob, wrong, ctx=ctx, verify=False).close()
    lacking = list(bases)
    lacking[victim] = None
    rs = np.random.RandomState(23)
    with container.open_delta_items(blob, lacking, ctx=ctx) as box:
        pick = np.array([i for i in rs.permutation(box.nitems) if i != victim][:50])
        pick[9] = victim
        plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs, pick)
        dst = Guarded(size, 4, salt=17)
        box.reserve(max_pick, int(plen.sum()))
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        st, position = ctx.sync_status(raise_on_error=False)
        assert st == rcx.E_CAPACITY and box.pick_of(position) == 9, (st, position)
        assert np.array_equal(dst.tensor.cpu().numpy(),
                              image_with(dst, [(at[k], np.frombuffer(items[int(i)], np.uint8)) for k, i in enumerate(pick) if int(i) != victim]))
    # pages against ONE reference page: the same object for every item
    page = np.random.RandomState(24).randint(0, 256, 4096).astype(np.uint8)
    pages = [(page.view(np.uint16) + np.uint16(k)).view(np.uint8).tobytes() for k in range(40)]
    one = page.tobytes()
    blob = container.pack_delta_items(pages, [one] * 40, widths=2, ctx=ctx)
    with container.open_delta_items(blob, [one] * 40, ctx=ctx) as box:
        assert box.base_cap == 4096
        pick = rs.permutation(40)
        plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs, pick)
        dst = Guarded(size, 4, salt=18)
        box.reserve(max_pick, int(plen.sum()))
        box.decode_into(d_pick, d_at, dev64([40]), dst.view, max_pick)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], np.frombuffer(pages[int(i)], np.uint8)) for k, i in enumerate(pick)]))


def test_open_delta_items_damage(ctx, state):
    """A checked container with one payload bit flipped in a stream that still decodes: verify raises ChecksumError with the
    item's number (a flip the decoder sees itself is latched at a pick of the item)."""
    items, bases, widths, ops, preds = state
    blob = container.pack_delta_items(items, bases, widths=widths, ops=ops, predict=preds, ctx=ctx, checksum=True)
    inner = container.parse_delta_items(blob)["inner"]
    head = len(blob) - len(inner["payload"])
    victim = 9
    sub = int(inner["sub_first"][victim])
    a, b = int(inner["offsets"][sub]), int(inner["offsets"][sub + 1])
    rs = np.random.RandomState(25)
    found = None
    for back in (5, 6, 7, 8, 10, 12, 16, 24, 32, (b - a) // 2):  # the first flip whose stream still decodes, and to other bytes
        flipped = bytearray(blob)
        flipped[head + b - back] ^= 0x10
        with container.open_delta_items(bytes(flipped), bases, ctx=ctx) as box:
            pick = rs.permutation(box.nitems)[:30]
            pick[4] = victim
            plen, at, size, max_pick, d_pick, d_at = picks_for(box, rs, pick)
            dst = Guarded(size, 4, salt=19)
            box.reserve(max_pick, int(plen.sum()))
            box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
            st, position = ctx.sync_status(raise_on_error=False)
            if st != rcx.OK:
                assert st == rcx.E_CORRUPT and pick[box.pick_of(position)] == victim, (back, st, position)
                continue
            try:
                box.verify(pick)
            except container.ChecksumError as e:
                assert e.index == victim and f"item {victim}" in str(e), str(e)
                found = back
                break
    assert found is not None, "no flipped bit left a stream that decodes to other bytes"


def test_open_delta_items_in_a_graph(state):
    """decode_into captured once -- lookup, decode and join as one chain -- and replayed with other picks."""
    items, bases, widths, ops, preds = state
    c = rcx.Context(0)
    try:
        blob = container.pack_delta_items(items, bases, widths=widths, ops=ops, predict=preds, ctx=c)
        fresh = rcx.Context(0)
        box = container.open_delta_items(blob, bases, ctx=fresh)
        n, max_pick = box.nitems, 48
        longest = int(box.lengths.max())
        box.reserve(max_pick, max_pick * longest)
        before = fresh.scratch_bytes()
        d_lengths = dev64(box.lengths)
        d_pick = torch.zeros(max_pick, dtype=torch.int64, device="cuda")
        d_at = torch.zeros_like(d_pick)
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = Guarded(max_pick * (longest + 32), 11, salt=21)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            box.decode_into(d_pick, d_at, d_count, dst.view, max_pick)
        for replay, (mul, add, count) in enumerate(((7, 3, 48), (11, 5, 10))):
            d_pick.copy_((torch.arange(max_pick, device="cuda") * mul + add) % n)
            d_len = d_lengths[d_pick]
            d_at.copy_(torch.cumsum(d_len + 17 + replay, 0) - d_len)
            d_count.fill_(count)
            dst.tensor.copy_(dst.before)
            g.replay()
            torch.cuda.synchronize()
            assert fresh.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            p, a = d_pick.cpu().numpy(), d_at.cpu().numpy()
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(a[k], np.frombuffer(items[int(p[k])], np.uint8)) for k in range(count)])), replay
        assert fresh.scratch_bytes() == before
        box.close()
        fresh.close()
    finally:
        c.close()
