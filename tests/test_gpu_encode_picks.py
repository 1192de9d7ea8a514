"""rcx_encode_picks_device on the GPU (include/rcx_encode_picks.h): item encode whose positions, lengths and count are read
from device memory, planned by kernels, capturable in a graph in front of rcx_decode_picks_device.  Expected streams are
rcx_encode_items_device's for the same bytes and the CPU oracle's item by item; what is latched is what
cpprcoder_amd/encode_picks.py's numpy model of the planner says.  Every buffer is guarded and compared whole: the source
is not written, the destination exactly in [0, comp_offsets[max_items]), the table in its max_items + 1 entries.  Nothing here
reads the reference's tree."""
import numpy as np
import pytest

from cpprcoder_amd import container, encode_picks as ep, picks, rcx, workloads
from encode_picks_cases import BAD, BAD_STATUS, PAST, TOP, back_to_back, edge_lengths, every_residue, padding_lengths, skew_lengths
from gpu_support import CODERS, Guarded, ctx, encode_items, encode_lanes, oracle_streams, shape_edges  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LONGEST = (1 << TOP) + 1
_POOL, _HOST = {}, {}


def make_items(lengths, names=("zipf", "uniform", "canterbury")):
    """Content rotates over the workloads; every item is its own slice of its workload."""
    at, items = [0] * len(names), []
    for i, n in enumerate(lengths):
        k = i % len(names)
        if names[k] not in _POOL:
            _POOL[names[k]] = workloads.by_name(names[k], 1 << 20, 77)
        if at[k] + int(n) > len(_POOL[names[k]]):
            at[k] = 0
        items.append(_POOL[names[k]][at[k]: at[k] + int(n)])
        at[k] += int(n)
    return items


def host_planned(ctx, key, items, coder):
    """rcx_encode_items_device's streams of these items (None for an empty one), made once per key and coder."""
    if (key, coder) not in _HOST:
        payload, offs = encode_items(ctx, items, coder)
        _HOST[key, coder] = [payload[int(offs[i]): int(offs[i + 1])].copy() if len(x) else None for i, x in enumerate(items)]
    return _HOST[key, coder]


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def source_of(items, at, size):
    data = np.zeros(size, np.uint8)
    for a, x in zip(at, items):
        data[int(a): int(a) + len(x)] = x
    return data


def run(ctx, coder, data, at, length, count, max_len, max_bytes, max_items=None, dst_cap=None, src_offset=0, dst_offset=0):
    """One call on guarded buffers -> (payload up to the total or dst_cap, comp_offsets uint64[max_items + 1], (status, position)).
    The source is unchanged, the table is written in its max_items + 1 entries, the destination in [0, min(total, dst_cap))."""
    max_items = len(length) if max_items is None else max_items
    src = Guarded(len(data), src_offset, data, salt=1)
    cap = ep.dst_bound(max_items, max_bytes, coder) if dst_cap is None else dst_cap
    dst = Guarded(cap, dst_offset, salt=2)
    offs = Guarded(8 * (max_items + 1), 0, salt=3)
    ep.encode_device(ctx, src.view, dev64(at), dev64(length), dev64([count]), dst.view, offs.view.view(torch.int64), max_len, max_bytes,
                     max_items=max_items, coder=coder)
    st = ctx.sync_status(raise_on_error=False)
    table = offs.view.view(torch.int64).cpu().numpy().astype(np.uint64)
    src.check(0, "encode picks src")
    offs.check(8 * (max_items + 1), "encode picks table")
    total = int(table[-1])
    assert np.all(np.diff(table.astype(np.int64)) >= 0), "the table decreases"
    if total <= cap:
        dst.check(total, "encode picks dst")
    return dst.view[: min(total, cap)].cpu().numpy(), table, st


def assert_streams(payload, table, want, label):
    """Stream k is want[k]; None or absent: an empty stream."""
    sizes = np.diff(table.astype(np.int64))
    for k in range(len(sizes)):
        w = want[k] if k < len(want) else None
        if w is None:
            assert sizes[k] == 0, (label, k, "should be empty")
        else:
            assert sizes[k] == len(w) and np.array_equal(payload[int(table[k]): int(table[k + 1])], w), (label, k, int(sizes[k]), len(w))


@pytest.mark.parametrize("coder", CODERS)
def test_parity_at_every_class_edge(ctx, oracle, coder):
    """Lengths on both sides of every class edge up to 2^17, and 1, 15 and 0, with sources at every residue mod 16, in a
    shuffled order: every stream is rcx_encode_items_device's and the oracle's."""
    lengths = edge_lengths()
    items = make_items(lengths)
    want = host_planned(ctx, "edges", items, coder)
    theirs = oracle_streams(oracle, items, coder)
    for i, (a, b) in enumerate(zip(want, theirs)):
        assert (a is None and b is None) or np.array_equal(a, b), ("the host-planned call against the oracle", i)
    order = np.random.RandomState(3 + coder).permutation(len(items))
    shuffled = [items[i] for i in order]
    at, size = every_residue([len(x) for x in shuffled])
    assert {int(a) % 16 for a in at} == set(range(16))
    payload, table, st = run(ctx, coder, source_of(shuffled, at, size), at, [len(x) for x in shuffled], len(items), LONGEST, sum(lengths))
    assert st[0] == rcx.OK, st
    assert_streams(payload, table, [want[i] for i in order], "edges")


@pytest.mark.parametrize("coder", CODERS)
def test_equal_aligned_items(ctx, coder):
    """130 items of 256 bytes back to back at an aligned address: the five-wave encoder's FULL pipeline on items, in two full
    units and one with holes."""
    items = make_items([256] * 130)
    want = host_planned(ctx, "equal", items, coder)
    at, size = back_to_back([256] * 130)
    payload, table, st = run(ctx, coder, source_of(items, at, size), at, [256] * 130, 130, 256, size)
    assert st[0] == rcx.OK, st
    assert_streams(payload, table, want, "equal")


@pytest.mark.parametrize("coder", CODERS)
def test_one_long_item_among_many_short_ones(ctx, coder):
    """One item of 2^17 + 1 bytes among 300 of 1 .. 64, overlapping sources and a repeat included."""
    lengths = skew_lengths()
    items = make_items(lengths)
    want = host_planned(ctx, "skew", items, coder)
    at, size = back_to_back(lengths)
    at, lens, want = list(at) + [at[137], at[3]], lengths + [1000, lengths[3]], want + [None, want[3]]
    want[-2] = host_planned(ctx, "skew+", [items[137][:1000]], coder)[0]  # (a prefix of the long item: the sources overlap)
    payload, table, st = run(ctx, coder, source_of(items, at, size), at, lens, len(lens), LONGEST, sum(lens))
    assert st[0] == rcx.OK, st
    assert_streams(payload, table, want, "skew")


@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("coder", CODERS)
def test_unit_padding(ctx, coder, n):
    """A class with exactly 63, 64 and 65 entries between two other classes."""
    lengths = padding_lengths(n)
    items = make_items(lengths)
    want = host_planned(ctx, ("pad", n), items, coder)
    at, size = every_residue(lengths)
    payload, table, st = run(ctx, coder, source_of(items, at, size), at, lengths, len(lengths), 1000, sum(lengths))
    assert st[0] == rcx.OK, st
    assert_streams(payload, table, want, ("pad", n))


@pytest.mark.parametrize("coder", CODERS)
def test_the_count_is_read_on_the_device(ctx, coder):
    """max_items = 1024 and every count around a wave's and the table's end; the entries at and behind the count hold 2^63 and
    are never read: nothing is latched, their streams are empty.  A count above max_items encodes max_items entries and latches
    RCX_E_CAPACITY at max_items."""
    rs = np.random.RandomState(50)
    lengths = rs.randint(0, 301, 1024)
    items = make_items(lengths)
    want = host_planned(ctx, "count", items, coder)
    at, size = back_to_back(lengths, gap=1)
    data = source_of(items, at, size)
    for count in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        meant = min(count, 1024)
        a, m = np.array(at, np.uint64), np.array(lengths, np.uint64)
        a[meant:], m[meant:] = PAST, PAST
        payload, table, st = run(ctx, coder, data, a, m, count, 300, int(lengths.sum()))
        assert st == ((rcx.OK, 0xFFFFFFFF) if count <= 1024 else (rcx.E_CAPACITY, 1024)), (count, st)
        assert_streams(payload, table, want[:meant], ("count", count))


def shape_points(cus):
    """max_items on both sides of every value at which a launch shape of the call changes.  The coding launches carry
    roundup64(max_items) + 64 * 21 entries: encode_lanes (csrc/rcx_launch.hpp) doubles the entries of a workgroup where that
    count passes cus x 1, 2, ... 32, the static coder changes its kernel where it passes 32768 (gpu_support.shape_edges).  The
    planner's grid (picks_grid) grows by a workgroup behind every 256 entries -- taken at the first -- and stops growing behind
    8 cus x 256."""
    entries = lambda m: ((m + 63) & ~63) + 64 * ep.CLASSES  # noqa: E731
    points = set()
    for edge in shape_edges(cus):
        m = (edge & ~63) - 64 * ep.CLASSES  # the last max_items whose launch has at most `edge` entries
        if m >= 1:
            assert entries(m) <= edge < entries(m + 1)
            points |= {m, m + 1}
    for m in (ep.PLAN_THREADS, 8 * cus * ep.PLAN_THREADS):
        points |= {m - 1, m, m + 1}
    return sorted(points)


@pytest.mark.parametrize("coder", CODERS)
def test_launch_shapes(ctx, coder):
    """Items of 64 bytes, up to 700 of them meant, under max_items on both sides of every value at which encode_lanes, the static
    coder's choice of kernel or the planner's launch changes shape.  Every meant stream is the host-planned call's, the rest of the
    table is the total, and nothing else is written."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count  # what rcx_ctx_create reads
    points = shape_points(cus)
    assert any(encode_lanes(((m + 63) & ~63) + 64 * ep.CLASSES, cus) != encode_lanes(((m + 1 + 63) & ~63) + 64 * ep.CLASSES, cus) for m in points)
    items = make_items([64] * 700)
    want = host_planned(ctx, "shapes", items, coder)
    sizes = np.array([len(s) for s in want], np.int64)
    d_want = torch.from_numpy(np.concatenate(want)).cuda()
    src = Guarded(64 * 700, 3, np.concatenate(items), salt=1)
    top = points[-1]
    d_at = torch.full((top,), -(1 << 63), dtype=torch.int64, device="cuda")
    d_len = d_at.clone()
    d_at[:700] = torch.arange(700, dtype=torch.int64, device="cuda") * 64
    d_len[:700] = 64
    dst = Guarded(ep.dst_bound(700, 64 * 700, coder), 5, salt=2)
    offs = Guarded(8 * (top + 1), 0, salt=3)
    for max_items in points:
        count = min(max_items, 700)
        dst.tensor.copy_(dst.before)
        offs.tensor.copy_(offs.before)
        ep.encode_device(ctx, src.view, d_at, d_len, dev64([count]), dst.view, offs.view.view(torch.int64), 64, 64 * 700, max_items=max_items, coder=coder)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK, max_items
        table = np.concatenate([[0], np.cumsum(sizes[:count]), np.full(max_items - count, sizes[:count].sum())])
        assert torch.equal(offs.view.view(torch.int64)[: max_items + 1].cpu(), torch.from_numpy(table)), max_items
        offs.check(8 * (max_items + 1), f"table, max_items {max_items}")
        total = int(table[-1])
        assert torch.equal(dst.view[:total], d_want[:total]), max_items
        dst.check(total, f"dst, max_items {max_items}")
    src.check(0, "src")


@pytest.mark.parametrize("where", [5, 200])
@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("coder", CODERS)
def test_bad_entries(ctx, coder, kind, where):
    """One bad entry among 300 good ones: the status and the position are the model's, the bad entry's stream is empty and every
    other stream is intact."""
    rs = np.random.RandomState(70)
    lengths = rs.randint(1, 3001, 300)
    items = make_items(lengths)
    want = list(host_planned(ctx, "bad", items, coder))
    at, size = back_to_back(lengths)
    a, m = np.array(at, np.uint64), np.array(lengths, np.uint64)
    a[where], m[where] = BAD[kind](size, 3000)
    want[where] = None
    model = ep.plan_numpy(a, m, 300, 3000, size, int(lengths.sum()), coder)
    assert (model["status"], model["position"]) == (BAD_STATUS[kind], where) and int(model["valid"].sum()) == 299
    payload, table, st = run(ctx, coder, source_of(items, at, size), a, m, 300, 3000, int(lengths.sum()))
    assert st == (model["status"], where), (kind, st)
    assert_streams(payload, table, want, kind)


@pytest.mark.parametrize("coder", CODERS)
def test_capacity(ctx, coder):
    """More valid bytes than max_bytes promised: every offset is 0, nothing is written, RCX_E_CAPACITY at the count.  A dst_cap one
    byte short of the total: RCX_E_CAPACITY at the count, the table whole, and no byte outside [d_dst, d_dst + dst_cap) written."""
    lengths = np.random.RandomState(80).randint(1, 2001, 200)
    items = make_items(lengths)
    want = host_planned(ctx, "capacity", items, coder)
    at, size = back_to_back(lengths)
    data, total_in = source_of(items, at, size), int(lengths.sum())
    payload, table, st = run(ctx, coder, data, at, lengths, 150, 2000, int(lengths[:150].sum()) - 1, dst_cap=ep.dst_bound(200, total_in, coder))
    assert st == (rcx.E_CAPACITY, 150) and not table.any() and len(payload) == 0, st
    assert ep.plan_numpy(at, lengths, 150, 2000, size, int(lengths[:150].sum()) - 1, coder)["over"]
    total = sum(len(s) for s in want)
    src, dst, offs = Guarded(size, 0, data, salt=1), Guarded(total - 1, 9, salt=2), Guarded(8 * 201, 0, salt=3)
    ep.encode_device(ctx, src.view, dev64(at), dev64(lengths), dev64([200]), dst.view, offs.view.view(torch.int64), 2000, total_in, coder=coder)
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CAPACITY, 200)
    table = offs.view.view(torch.int64).cpu().numpy().astype(np.uint64)
    assert np.array_equal(np.diff(table.astype(np.int64)), [len(s) for s in want]) and int(table[-1]) == total
    dst.check(total - 1, "a destination one byte short")
    got = dst.view.cpu().numpy()
    for k in range(199):  # (the last stream is the one that does not fit)
        assert np.array_equal(got[int(table[k]): int(table[k + 1])], want[k]), k


def test_carry_runs_through_the_second_pass(ctx, oracle):
    """Blocks whose carry runs through more bytes than the five-wave encoder keeps are marked and coded again by the one-wave
    kernel, which finds its entries, strides and slot bases through the same units: the streams are the oracle's."""
    import carry_runs
    runs = [0, 3, 20, 30, 40, 70, 300, 0, 0, 45, 0, 1000]  # (tests/test_gpu_parity.py's blocks: these seeds have their runs)
    items = [carry_runs.carry_run_block(4096, r, 100 + i) if r else workloads.uniform(4096, 100 + i) for i, r in enumerate(runs)]
    items += make_items([100, 5000, 33])
    want = oracle_streams(oracle, items, 0)
    lengths = [len(x) for x in items]
    at, size = every_residue(lengths)
    payload, table, st = run(ctx, 0, source_of(items, at, size), at, lengths, len(items), 5000, sum(lengths))
    assert st[0] == rcx.OK, st
    assert_streams(payload, table, want, "carry runs")
    positions = ep.plan_numpy(at, lengths, len(items), 5000, size, sum(lengths))["positions"]
    assert ctx.last_redo(positions) >= sum(r > 64 for r in runs)


def device_set(lengths, gap=3):
    items = make_items(lengths)
    at, size = back_to_back(lengths, gap=gap, first=1)
    return items, at, torch.from_numpy(source_of(items, at, size)).cuda()


@pytest.mark.parametrize("coder", CODERS)
def test_round_trip_on_the_device(ctx, coder):
    """Encode picks, then rcx_decode_picks_device over the streams where they lie, nstreams = max_items: nothing is downloaded in
    between, and every meant item is back where the decode tables put it."""
    lengths = np.array(edge_lengths()[:-4] + [1000, 0, 77] * 20)
    items, at, d_src = device_set(lengths)
    n, max_items = len(items), len(items) + 9
    d_at, d_len = dev64(list(at) + [PAST] * 9), dev64(list(lengths) + [PAST] * 9)
    d_count = dev64([n])
    d_comp = torch.empty(ep.dst_bound(max_items, int(lengths.sum()), coder), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(max_items + 1, dtype=torch.int64, device="cuda")
    out = Guarded(d_src.numel(), 6, salt=4)
    ep.encode_device(ctx, d_src, d_at, d_len, d_count, d_comp, d_offs, int(lengths.max()), int(lengths.sum()), coder=coder)
    d_pick = torch.arange(max_items, dtype=torch.int64, device="cuda")
    picks.decode_device(ctx, d_comp, d_comp.numel(), d_offs, d_pick, d_at, d_len, d_count, out.view, int(lengths.max()), coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    want = out.before.cpu().numpy().copy()
    for a, x in zip(at, items):
        want[out.at + int(a): out.at + int(a) + len(x)] = x
    assert np.array_equal(out.tensor.cpu().numpy(), want)


@pytest.mark.parametrize("coder", CODERS)
def test_graph_capture_and_replay(coder):
    """Both reservations, then encode and decode captured in one graph; three replays, the positions, lengths and count rewritten
    by device ops between them.  Every replay's output is the meant items, and the context's scratch stays what the two
    reservations made it, which is what scratch_bytes says for a fresh context."""
    max_items, max_len, max_bytes = 400, 3000, 400 * 2000
    pool = torch.from_numpy(workloads.by_name("zipf", 1 << 20, 5)).cuda()
    c = rcx.Context(0)
    try:
        ep.reserve(c, max_items, max_len, max_bytes, coder)
        assert c.scratch_bytes() == ep.scratch_bytes(max_items, max_len, max_bytes, coder)
        picks.reserve(c, max_items, max_len, coder)
        before = c.scratch_bytes()
        d_at = torch.zeros(max_items, dtype=torch.int64, device="cuda")
        d_len, d_out_at = torch.zeros_like(d_at), torch.zeros_like(d_at)
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_pick = torch.arange(max_items, dtype=torch.int64, device="cuda")
        d_comp = torch.empty(ep.dst_bound(max_items, max_bytes, coder), dtype=torch.uint8, device="cuda")
        d_offs = torch.zeros(max_items + 1, dtype=torch.int64, device="cuda")
        out = Guarded(max_bytes + 32 * max_items, 11, salt=12)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ep.encode_device(c, pool, d_at, d_len, d_count, d_comp, d_offs, max_len, max_bytes, coder=coder)
            picks.decode_device(c, d_comp, d_comp.numel(), d_offs, d_pick, d_out_at, d_len, d_count, out.view, max_len, coder=coder)
        k = torch.arange(max_items, dtype=torch.int64, device="cuda")
        for replay, (mul, add, count) in enumerate(((7, 3, 400), (11, 5, 100), (13, 1, 333))):
            # device only: new lengths (some 0, some on a class edge), new sources, new destinations, a new count
            d_len.copy_((k * mul * 97 + add * 131) % 2001 * ((k + replay) % 7 != 0))
            d_at.copy_((k * mul * 2503 + add) % ((1 << 20) - 3000))
            d_out_at.copy_(torch.cumsum(d_len + 5 + replay, 0) - d_len)
            d_count.fill_(count)
            d_len[count:] = -(1 << 63)
            out.tensor.copy_(out.before)
            g.replay()
            torch.cuda.synchronize()
            assert c.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            want = out.before.clone()
            a, m, o = d_at.cpu().numpy(), d_len.cpu().numpy(), d_out_at.cpu().numpy()
            host_pool = pool.cpu().numpy()
            image = want.cpu().numpy()
            for i in range(count):
                image[out.at + int(o[i]): out.at + int(o[i]) + int(m[i])] = host_pool[int(a[i]): int(a[i]) + int(m[i])]
            assert np.array_equal(out.tensor.cpu().numpy(), image), replay
            assert int(d_offs[count]) == int(d_offs[max_items]) and int(d_offs[count]) > 0
        assert c.scratch_bytes() == before
    finally:
        c.close()


@pytest.mark.parametrize("coder", [rcx.CODER_ADAPTIVE, rcx.CODER_RANS8])
def test_pack_items_device(ctx, coder):
    """pack_items_device(...).to_bytes() is the container pack_items writes for the same items, unpack_items reads it, and
    decode_into -- picks on the device, nothing downloaded -- gives the picked items."""
    lengths = np.array([0, 1, 16, 17, 65, 300, 1024, 1025, 3000, 5000, 20_000] * 3)
    items, at, d_src = device_set(lengths)
    n, max_items = len(items), len(items) + 5
    d_at, d_len = dev64(list(at) + [PAST] * 5), dev64(list(lengths) + [PAST] * 5)
    box = container.pack_items_device(ctx, d_src, d_at, d_len, dev64([n]), max_items, 20_000, int(lengths.sum()), coder=coder)
    rs = np.random.RandomState(9)
    pick = np.concatenate([rs.permutation(n), [3, 3, n + 2]])  # (the last names a stream behind the count: skipped and latched)
    plen = np.array([lengths[int(i)] if i < n else 1 for i in pick], np.uint64)
    doffs = rcx.item_offsets(plen)
    out = Guarded(int(doffs[-1]), 2, salt=7)
    box.reserve(len(pick))
    box.decode_into(dev64(pick), dev64(doffs[:-1]), dev64([len(pick)]), out.view)
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, len(pick) - 1)
    want = out.before.cpu().numpy().copy()
    for k, i in enumerate(pick[:-1]):
        want[out.at + int(doffs[k]): out.at + int(doffs[k + 1])] = items[int(i)]
    assert np.array_equal(out.tensor.cpu().numpy(), want)
    blob = box.to_bytes()
    assert blob == container.pack_items([x.tobytes() for x in items], coder=coder, ctx=ctx)
    assert container.unpack_items(blob, ctx=ctx) == [x.tobytes() for x in items]


@pytest.mark.parametrize("coder", CODERS)
def test_host_buffers(ctx, coder):
    """rcx_encode_picks: the same on host buffers, every entry meant; behind a latched failure the good entries' streams are there
    all the same and the bad one's is empty."""
    lengths = np.random.RandomState(110).randint(0, 3001, 120)
    items = make_items(lengths)
    want = list(host_planned(ctx, "host", items, coder))
    at, size = every_residue(lengths)
    data = source_of(items, at, size)
    payload, table, st = ep.encode(ctx, data, at, lengths, 3000, coder=coder)
    assert st == rcx.OK
    assert_streams(payload, table, want, "host buffers")
    a, m = np.array(at, np.uint64), np.array(lengths, np.uint64)
    a[7], m[7] = size - 3, 4
    want[7] = None
    payload, table, st = ep.encode(ctx, data, a, m, 3000, coder=coder)
    assert st == rcx.E_CAPACITY
    assert_streams(payload, table, want, "host buffers, one bad entry")
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # (the call took the latch with it)
