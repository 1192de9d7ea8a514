"""rcx_decode_picks_device on the GPU (include/rcx_picks.h): item decode whose picks, destinations, count and stored flags
are read from device memory, planned by kernels, capturable in a graph.  Expected bytes are the items themselves, whose
streams come from the CPU oracle item by item; what is latched is what cpprcoder_amd/picks.py's numpy model of the planner
says.  Every output buffer is guarded: a whole-buffer comparison sees any byte written outside the meant ranges.  Nothing
here reads the reference's tree."""
import numpy as np
import pytest

from cpprcoder_amd import container, picks, rcx, stored as stored_calls, stored_items, workloads
from gpu_support import CODERS, HEAD, Guarded, ctx, decode_quads, oracle_streams  # noqa: F401
from gpu_support import decode_items as host_planned_decode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SPECIAL = (0, 1, 15, 16, 17, 63, 64, 65)
LONGEST = 70_000
PAST = -(1 << 63)  # 2^63 as the int64 the tables hold: what entries past the count are filled with

_POOLS, _BATCH = {}, {}


def make_items(lengths, names=("zipf", "uniform", "canterbury")):
    """Content rotates over the workloads; every item is its own slice of its workload."""
    need = [sum(int(n) for n in lengths[k::len(names)]) for k in range(len(names))]
    at, items = [0] * len(names), []
    for i, n in enumerate(lengths):
        k = i % len(names)
        if names[k] not in _POOLS or len(_POOLS[names[k]]) < need[k]:
            _POOLS[names[k]] = workloads.by_name(names[k], max(need[k], 1 << 20), 77)
        items.append(_POOLS[names[k]][at[k]: at[k] + int(n)])
        at[k] += int(n)
    return items


def compact(streams):
    offs = np.zeros(len(streams) + 1, np.uint64)
    np.cumsum([0 if s is None else len(s) for s in streams], out=offs[1:])
    parts = [s for s in streams if s is not None]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs


def ragged_batch(oracle, coder):
    """About 300 items: the special lengths three times, random lengths up to 5000, one item of 70 000 bytes; and the oracle's
    streams for them (made once per coder)."""
    if coder not in _BATCH:
        rs = np.random.RandomState(2031)
        lengths = np.concatenate([np.repeat(SPECIAL, 3), rs.randint(1, 5001, 275), [LONGEST]])
        rs.shuffle(lengths)
        items = make_items(lengths)
        _BATCH[coder] = (items, oracle_streams(oracle, items, coder))
    return _BATCH[coder]


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def scattered(lengths, rs, gap=True):
    """Where each entry's bytes go: the entries take their places in a shuffled order, each start at the next residue mod 16
    (with a gap of guard bytes in front of it) -> (at uint64[], the size of the buffer)."""
    at = np.zeros(len(lengths), np.uint64)
    cursor = 0
    for r, k in enumerate(rs.permutation(len(lengths))):
        if gap:
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


def run_picks(ctx, coder, payload, offs, pick, at, length, count, dst, max_len, stored=None, dst_cap=None):
    """One call on guarded inputs and the guarded output `dst` -> (status, position); the inputs are unchanged."""
    comp = Guarded(len(payload), 1, payload, salt=4)
    table = Guarded(8 * len(offs), 0, np.asarray(offs).astype(np.int64).view(np.uint8), salt=5)
    d_stored = None if stored is None else torch.from_numpy(np.asarray(stored, dtype=np.uint8)).cuda()
    d_pick, d_at, d_len, d_count = dev64(pick), dev64(at), dev64(length), dev64([count])
    picks.decode_device(ctx, comp.view, len(payload), table.view.view(torch.int64), d_pick, d_at, d_len, d_count, dst.view, max_len, stored=d_stored,
                        coder=coder, dst_cap=dst_cap)
    st = ctx.sync_status(raise_on_error=False)
    comp.check(0, "picks comp")
    table.check(0, "picks table")
    return st


@pytest.mark.parametrize("coder", CODERS)
def test_parity(ctx, oracle, coder):
    """Unordered picks with repeats to distinct outputs at every residue mod 16: every output is the item's bytes and every
    other byte of the buffer keeps its guard pattern; laid out back to back, the whole buffer is what the host-planned call
    writes."""
    items, want = ragged_batch(oracle, coder)
    payload, offs = compact(want)
    rs = np.random.RandomState(40 + coder)
    n = len(items)
    pick = np.concatenate([rs.permutation(n), rs.randint(0, n, 60), [int(np.argmax([len(x) for x in items]))] * 2])
    lengths = np.array([len(items[int(i)]) for i in pick], np.uint64)
    at, size = scattered(lengths, rs)
    assert {int(a) % 16 for a, m in zip(at, lengths) if m} == set(range(16))
    dst = Guarded(size, 5, salt=6)
    st = run_picks(ctx, coder, payload, offs, pick, at, lengths, len(pick), dst, LONGEST)
    assert st[0] == rcx.OK, st
    got = dst.tensor.cpu().numpy()
    for k, i in enumerate(pick):
        assert np.array_equal(got[dst.at + int(at[k]): dst.at + int(at[k]) + int(lengths[k])], items[int(i)]), (k, int(i))
    assert np.array_equal(got, image_with(dst, [(at[k], items[int(i)]) for k, i in enumerate(pick)])), "a byte outside the picked ranges changed"
    # back to back: the same bytes as rcx_decode_items_device on the same picks
    doffs = rcx.item_offsets(lengths)
    mine, theirs = Guarded(int(doffs[-1]), 3, salt=7), Guarded(int(doffs[-1]), 3, salt=7)
    st = run_picks(ctx, coder, payload, offs, pick, doffs[:-1], lengths, len(pick), mine, LONGEST)
    assert st[0] == rcx.OK, st
    ctx.decode_items_device(torch.from_numpy(payload).cuda(), len(payload), dev64(offs), doffs, theirs.view, pick=pick, coder=coder)
    ctx.sync_status()
    assert torch.equal(mine.tensor, theirs.tensor)
    assert {(mine.at + int(o)) % 16 for o in doffs[:-1]} == set(range(16))


@pytest.mark.parametrize("coder", CODERS)
def test_the_count_is_read_on_the_device(ctx, oracle, coder):
    """max_pick = 1024 and every count around a wave's and the table's end; the entries past the count hold 2^63 and are never
    read: nothing is latched and nothing outside the meant ranges is written.  A count above max_pick decodes max_pick entries
    and latches RCX_E_CAPACITY at max_pick."""
    items, want = ragged_batch(oracle, coder)
    payload, offs = compact(want)
    rs = np.random.RandomState(50 + coder)
    short = [i for i, x in enumerate(items) if len(x) <= 5000]
    pick = rs.choice(short, 1024)
    lengths = np.array([len(items[int(i)]) for i in pick], np.uint64)
    at, size = scattered(lengths, rs)
    for count in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        meant = min(count, 1024)
        p, a, m = (np.asarray(x).astype(np.int64) for x in (pick, at, lengths))
        p[meant:], a[meant:], m[meant:] = PAST, PAST, PAST
        dst = Guarded(size, 9, salt=count)
        st = run_picks(ctx, coder, payload, offs, p.view(np.uint64), a.view(np.uint64), m.view(np.uint64), count, dst, 5000)
        assert st == ((rcx.OK, 0xFFFFFFFF) if count <= 1024 else (rcx.E_CAPACITY, 1024)), (count, st)
        assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(at[k], items[int(pick[k])]) for k in range(meant)])), count


def shape_points(cus):
    """Entry counts on both sides of every value at which a launch shape of the call changes: decode_quads (csrc/rcx_launch.hpp)
    doubles the entries of a wave behind 4 cus x 1, 2, 4, 8; wide_workgroups has no such value; the planner's grid
    (csrc/rcx_picks_api.hpp, picks_grid) grows by a workgroup behind every 256 entries -- taken at the first -- and stops
    growing, so that its threads go round, behind 8 cus x 256; its waves have 64 lanes."""
    edges = [4 * cus * k for k in (1, 2, 4, 8)] + [64, picks.PLAN_THREADS, 8 * cus * picks.PLAN_THREADS]
    assert all(decode_quads(m, cus) != decode_quads(m + 1, cus) for m in edges[:4])
    return sorted({m + d for m in edges for d in (-1, 0, 1)})


@pytest.mark.parametrize("coder", CODERS)
def test_launch_shapes(ctx, oracle, coder):
    """Items of 64 bytes; max_pick, and separately the count under the largest max_pick, on both sides of every value at which
    decode_quads or the planner's launch changes shape.  Every meant entry decodes, and nothing else is written."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count  # what rcx_ctx_create reads
    points = shape_points(cus)
    items = make_items([64] * 12)
    payload, offs = compact(oracle_streams(oracle, items, coder))
    d_items = torch.from_numpy(np.stack(items)).cuda()
    d_comp, d_offs = torch.from_numpy(payload).cuda(), dev64(offs)
    top = points[-1]
    rs = np.random.RandomState(60 + coder)
    d_pick = dev64(rs.randint(0, len(items), top))
    d_at = torch.arange(top, dtype=torch.int64, device="cuda") * 64 + 3
    d_len = torch.full((top,), 64, dtype=torch.int64, device="cuda")
    guard = Guarded(top * 64 + 3, 7, salt=8)
    rows = d_items[d_pick]
    for max_pick, count in [(m, m) for m in points] + [(top, m) for m in points[:-1]]:
        guard.tensor.copy_(guard.before)
        picks.decode_device(ctx, d_comp, len(payload), d_offs, d_pick, d_at, d_len, dev64([count]), guard.view, 64, max_pick=max_pick, coder=coder)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK, (max_pick, count)
        want = guard.before.clone()
        want[guard.at + 3: guard.at + 3 + 64 * count] = rows[:count].reshape(-1)
        assert torch.equal(guard.tensor, want), (max_pick, count)


@pytest.mark.parametrize("coder", CODERS)
def test_graph_capture_and_replay(oracle, coder):
    """Reserve, capture the call once (a linear graph on one stream), replay three times; between the replays the picks, the
    destinations and the count are rewritten by torch ops on the device only.  Every replay's output is the items its picks
    name, and the context's scratch is what it was before the capture."""
    items, want = ragged_batch(oracle, coder)
    payload, offs = compact(want)
    n, max_pick = len(items), 512
    c = rcx.Context(0)
    try:
        picks.reserve(c, max_pick, LONGEST, coder)
        before = c.scratch_bytes()
        assert before == picks.scratch_bytes(max_pick, LONGEST, coder)
        d_comp, d_offs = torch.from_numpy(payload).cuda(), dev64(offs)
        d_lengths = dev64([len(x) for x in items])
        d_pick = torch.zeros(max_pick, dtype=torch.int64, device="cuda")
        d_at, d_len = torch.zeros_like(d_pick), torch.zeros_like(d_pick)
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        size = max_pick * 5016 + LONGEST * 8
        dst = Guarded(size, 11, salt=12)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            picks.decode_device(c, d_comp, len(payload), d_offs, d_pick, d_at, d_len, d_count, dst.view, LONGEST, coder=coder)
        for replay, (mul, add, count) in enumerate(((7, 3, 512), (11, 5, 100), (13, 1, 333))):
            # device only: new picks, their lengths, destinations with a gap that moves the residues, a new count
            d_pick.copy_((torch.arange(max_pick, device="cuda") * mul + add) % n)
            d_len.copy_(d_lengths[d_pick])
            d_at.copy_(torch.cumsum(d_len + 17 + replay, 0) - d_len)
            d_count.fill_(count)
            dst.tensor.copy_(dst.before)
            g.replay()
            torch.cuda.synchronize()
            assert c.sync_status(raise_on_error=False)[0] == rcx.OK, replay
            p, a = d_pick.cpu().numpy(), d_at.cpu().numpy()
            assert int(a[count - 1]) + LONGEST <= size
            assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, [(a[k], items[int(p[k])]) for k in range(count)])), replay
        assert c.scratch_bytes() == before
    finally:
        c.close()


def stored_set(oracle, coder):
    """The ragged batch as a mixed set: every third item with bytes is stored (its stream is the item).  One more stream, the
    last, is FLAGGED stored but is a coder's stream, shorter than its item: picking it is the stored length mismatch."""
    items, want = ragged_batch(oracle, coder)
    flags = np.array([1 if len(x) and i % 3 == 1 else 0 for i, x in enumerate(items)], np.uint8)
    streams = [items[i] if flags[i] else want[i] for i in range(len(items))]
    liar = next(i for i, x in enumerate(items) if 3000 < len(x) <= 5000 and i % 3 == 0 and len(want[i]) != len(x))
    items, streams, flags = items + [items[liar]], streams + [want[liar]], np.concatenate([flags, [1]])
    return items, streams, flags


BAD = {  # kind -> (pick, at, length) of the bad entry, given the set's size, the buffer's size and the liar's index
    "bad pick": lambda n, size, liar: (n, 64, 100),
    "length above max_len": lambda n, size, liar: (0, 64, 5001),
    "output past dst_cap": lambda n, size, liar: (3, size - 50, 100),
    "stored length mismatch": lambda n, size, liar: (liar, 64, 4000),
}


@pytest.mark.parametrize("where", [5, 200])
@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("coder", CODERS)
def test_bad_entries(ctx, oracle, coder, kind, where):
    """One bad entry among 300 good ones, coded and stored: the status and the position are the model's, the bad entry's
    destination keeps its guard bytes, and every good entry decodes."""
    items, streams, flags = stored_set(oracle, coder)
    payload, offs = compact(streams)
    rs = np.random.RandomState(70 + coder)
    n, liar = len(items), len(items) - 1
    good = [i for i in range(n - 1) if len(items[i]) <= 5000]
    pick = rs.choice(good, 300).astype(np.uint64)
    lengths = np.array([len(items[int(i)]) for i in pick], np.uint64)
    at, size = scattered(lengths, rs)
    at += 8192  # (room for the bad entry's own destination in front)
    size += 8192
    pick[where], at[where], lengths[where] = BAD[kind](n, size, liar)
    if kind == "stored length mismatch":
        lengths[where] = len(items[liar])  # its output length; its stream is shorter
    model = picks.plan_numpy(pick, at, lengths, 300, 5000, n, size, stored=flags, comp_offsets=offs, comp_size=len(payload))
    assert model["status"] == (rcx.E_CAPACITY if kind == "output past dst_cap" else rcx.E_CORRUPT) and model["position"] == where
    dst = Guarded(size, 2, salt=13)
    st = run_picks(ctx, coder, payload, offs, pick, at, lengths, 300, dst, 5000, stored=flags)
    assert st == (model["status"], where), (kind, st)
    assert {picks.CODED, picks.STORED_LONG, picks.STORED_SHORT} <= set(model["route"])
    entries = [(at[k], items[int(pick[k])]) for k in range(300) if model["route"][k]]
    assert len(entries) >= 270
    assert np.array_equal(dst.tensor.cpu().numpy(), image_with(dst, entries)), kind


@pytest.mark.parametrize("coder", CODERS)
def test_stored_flags_never_leave_the_device(ctx, oracle, coder):
    """rcx_encode_items_device, rcx_stored_mix_items_device, then the new call with the flags where the mix left them: no
    download in between, and the result is the source.  The same picks through rcx_stored_decode_device with the downloaded
    flags give the same bytes."""
    lengths = np.array([0, 1, 16, 17, 64, 300, 1024, 1025, 2000, 4097, 5000, 40_000] * 4)
    items = make_items(lengths, names=("uniform", "zipf"))  # incompressible and compressible, by turns
    soffs = rcx.item_offsets(lengths)
    n = len(items)
    d_src = torch.from_numpy(np.concatenate(items)).cuda()
    d_comp = torch.empty(rcx.encode_items_bound(soffs, coder), dtype=torch.uint8, device="cuda")
    d_coffs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_mixed = torch.empty(d_src.numel(), dtype=torch.uint8, device="cuda")
    d_moffs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rs = np.random.RandomState(80 + coder)
    pick = rs.permutation(n)
    plen = lengths[pick].astype(np.uint64)
    doffs = rcx.item_offsets(plen)
    mine, theirs = Guarded(int(doffs[-1]), 1, salt=14), Guarded(int(doffs[-1]), 1, salt=14)
    ctx.encode_items_device(d_src, soffs, d_comp, d_coffs, coder=coder)
    stored_items.mix_items_device(ctx, d_src, soffs, d_comp, d_comp.numel(), d_coffs, 0, d_mixed, d_moffs, d_flags)
    picks.decode_device(ctx, d_mixed, d_mixed.numel(), d_moffs, dev64(pick), dev64(doffs[:-1]), dev64(plen), dev64([n]), mine.view, 40_000,
                        stored=d_flags, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    flags = d_flags.cpu().numpy()
    assert flags.any() and not flags.all(), "the batch should hold items of both kinds"
    assert np.array_equal(mine.tensor.cpu().numpy(), image_with(mine, [(doffs[k], items[int(i)]) for k, i in enumerate(pick)]))
    stored_calls.decode_device(ctx, d_mixed, d_mixed.numel(), d_moffs, flags, doffs, theirs.view, pick=pick.astype(np.uint64), coder=coder)
    ctx.sync_status()
    assert torch.equal(mine.tensor, theirs.tensor)


@pytest.mark.parametrize("kind", ["truncated", "payload bit"])
@pytest.mark.parametrize("coder", CODERS)
def test_damaged_streams(oracle, coder, kind):
    """The families of tests/test_gpu_damaged.py on three picks: a stream cut short and a flipped payload bit.  These are inputs
    the decoders answer with a status or with some bytes, never otherwise; status and position are the host-planned call's, and
    every undamaged pick decodes."""
    items, want = ragged_batch(oracle, coder)
    rs = np.random.RandomState(90 + coder)
    mid = [i for i, x in enumerate(items) if 800 <= len(x) <= 5000]
    victims = [int(v) for v in rs.choice(mid, 3, replace=False)]
    streams = list(want)
    for v in victims:
        s = want[v].copy()
        if kind == "truncated":
            s = s[: len(s) - 40]
        else:
            s[HEAD[coder] + 4 + (len(s) - HEAD[coder] - 4) // 2] ^= 0x10
            s = np.concatenate([s, rs.randint(0, 256, 3 * len(items[v])).astype(np.uint8)])  # (as there: the decoder does not run dry)
        streams[v] = s
    payload, offs = compact(streams)
    pick = np.concatenate([rs.permutation(len(items))[:150], victims])
    rs.shuffle(pick)
    lengths = np.array([len(items[int(i)]) for i in pick], np.uint64)
    doffs = rcx.item_offsets(lengths)
    c = rcx.Context(0)
    try:
        theirs, st_host, bad_host = host_planned_decode(c, payload, offs, lengths, coder, pick=pick.astype(np.uint64))
        dst = Guarded(int(doffs[-1]), 0, salt=15)
        st = run_picks(c, coder, payload, offs, pick, doffs[:-1], lengths, len(pick), dst, LONGEST)
        assert st[0] == st_host and (st_host == rcx.OK or st[1] == bad_host), (kind, st, st_host, bad_host)
        if kind == "truncated":
            assert st_host == rcx.E_CORRUPT
        got = dst.view.cpu().numpy()
        for k, i in enumerate(pick):
            if int(i) not in victims:
                assert np.array_equal(got[int(doffs[k]): int(doffs[k + 1])], items[int(i)]), (kind, k)
            elif st_host == rcx.OK:
                assert np.array_equal(got[int(doffs[k]): int(doffs[k + 1])], theirs[k]), (kind, k, "the host-planned call's bytes")
    finally:
        c.close()


@pytest.mark.parametrize("made", ["stored", "plain", "checked"])
def test_open_items(ctx, made):
    """A container opened once on the device; decode_into a scattered layout gives, entry by entry, what unpack gives for the
    same picks -- the stored item container (typed items of width 1), a plain RCXI one and one with checksums, which verify()
    checks over a contiguous result."""
    lengths = [0, 1, 16, 65, 300, 1024, 1025, 3000, 5000, 20_000] * 3
    items = [x.tobytes() for x in make_items(lengths, names=("uniform", "zipf"))]
    if made == "stored":
        blob = container.pack_typed_items(items, widths=1, stored=True, ctx=ctx)
        assert container.parse_typed_items(blob).get("stored") is not None
        unpack = container.unpack_typed_items
    else:
        blob = container.pack_items(items, ctx=ctx, checksum=made == "checked")
        unpack = container.unpack_items
    rs = np.random.RandomState(17)
    pick = np.concatenate([rs.permutation(len(items)), rs.randint(0, len(items), 10)])
    want = unpack(blob, pick=[int(i) for i in pick], ctx=ctx)
    plen = np.array([lengths[int(i)] for i in pick], np.uint64)
    at, size = scattered(plen, rs)
    dst = Guarded(size, 4, salt=16)
    with container.open_items(blob, ctx=ctx) as box:
        assert box.nitems == len(items) and box.max_len == 20_000 and (box.d_stored is not None) == (made == "stored")
        max_pick = len(pick) + 7
        d_pick = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
        d_at = torch.full((max_pick,), PAST, dtype=torch.int64, device="cuda")
        d_pick[: len(pick)], d_at[: len(pick)] = dev64(pick), dev64(at)
        box.reserve(max_pick)
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        got = dst.tensor.cpu().numpy()
        for k in range(len(pick)):
            assert got[dst.at + int(at[k]): dst.at + int(at[k]) + int(plen[k])].tobytes() == want[k], (made, k)
        assert np.array_equal(got, image_with(dst, [(at[k], np.frombuffer(want[k], np.uint8)) for k in range(len(pick))]))
        # a pick that names no item is skipped and latched at its position
        d_pick[3] = len(items)
        box.decode_into(d_pick, d_at, dev64([len(pick)]), dst.view, max_pick)
        assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, 3)
        if made == "checked":
            doffs = rcx.item_offsets(plen)
            flat = torch.zeros(int(doffs[-1]), dtype=torch.uint8, device="cuda")
            d_pick[3] = int(pick[3])
            box.decode_into(d_pick, dev64(doffs[:-1]), dev64([len(pick)]), flat, len(pick))
            ctx.sync_status()
            box.verify(flat, pick)
            k = next(k for k in range(len(pick)) if plen[k] >= 2)
            flat[int(doffs[k]) + 1] ^= 1
            with pytest.raises(container.ChecksumError):
                box.verify(flat, pick)


@pytest.mark.parametrize("coder", CODERS)
def test_host_buffers(ctx, oracle, coder):
    """rcx_decode_picks: the same on host buffers, every entry meant.  dst goes to the device and comes back as a whole, so what
    no pick writes keeps its bytes; behind a latched failure the good entries are written all the same."""
    items, streams, flags = stored_set(oracle, coder)
    payload, offs = compact(streams)
    rs = np.random.RandomState(110 + coder)
    good = [i for i in range(len(items) - 1) if len(items[i]) <= 5000]
    pick = rs.choice(good, 120).astype(np.uint64)
    lengths = np.array([len(items[int(i)]) for i in pick], np.uint64)
    at, size = scattered(lengths, rs)
    pattern = ((np.arange(size) * 29 + 7) % 253 + 1).astype(np.uint8)
    dst = pattern.copy()
    assert picks.decode(ctx, payload, offs, pick, at, lengths, 5000, dst, stored=flags, coder=coder) == rcx.OK
    want = pattern.copy()
    for k, i in enumerate(pick):
        want[int(at[k]): int(at[k]) + int(lengths[k])] = items[int(i)]
    assert np.array_equal(dst, want)
    pick[7] = len(items)  # names no stream
    if lengths[7] == 0:
        lengths[7] = 1
    dst = pattern.copy()
    assert picks.decode(ctx, payload, offs, pick, at, lengths, 5000, dst, stored=flags, coder=coder) == rcx.E_CORRUPT
    want[int(at[7]): int(at[7]) + int(lengths[7])] = pattern[int(at[7]): int(at[7]) + int(lengths[7])]
    assert np.array_equal(dst, want)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # (the call took the latch with it)
