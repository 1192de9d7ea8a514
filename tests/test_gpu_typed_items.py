"""The typed stage per item on the GPU (include/rcx_typed_items.h; csrc/rcx_typed_items.hpp) against its numpy expectation
(tests/typed_items_cases.py: every item one superblock of predict_cases), and the RCXJ container and the named tensors on
top of it against the CPU oracle.

The kernels spread units of 16 elements over all items of a class (width, predictor): a row is 256 units, a workgroup step
16 / w rows, what is not a unit goes byte by byte, and join with a predictor gives a wave whole items, tile (1024 elements) by
tile.  The batches sit on both sides of every border of that -- item lengths around one element, one unit, 64 and 256 units,
one step, one and two tiles; small neighbours of every class inside one row; runs of empty items; large items beside small
ones -- at every pair of source and destination offsets of (0, 1, 3, 8, 15), every buffer guarded, with random bytes, the
elements -k and a ramp across 2^32; then 65 535 to 65 537 items, and 8 MiB + 5 bytes where the fixed grids loop.
"""
import zlib

import numpy as np
import pytest

import planes_cases as pc
import predict_cases as pr
import typed_items_cases as tc
from cpprcoder_amd import container, predict, rcx, typed_items
from gpu_support import CODERS, Guarded, assert_same_items, ctx, oracle_decode_one, oracle_streams, run_filter  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20259).randint(0, 256, (9 << 20) + 64, dtype=np.uint8)


def run(ctx, join, x, offs, widths, preds, src_offset=0, dst_offset=0):
    """gpu_support.run_filter of one typed item call over a batch that fills the buffer."""
    assert len(offs) == 1 or (int(offs[0]) == 0 and int(offs[-1]) == len(x))
    fn = typed_items.join_device if join else typed_items.split_device
    return run_filter(ctx, lambda src, dst: fn(ctx, src, offs, widths, preds, dst), f"typed items {'join' if join else 'split'} nitems={len(widths)}", x,
                      src_offset, dst_offset)


# ---- the kernels against numpy ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return tc.kernel_cases()


@pytest.mark.parametrize("kind", tc.KINDS)
def test_split_and_join_against_numpy(ctx, noise, cases, kind):
    assert len(cases) == 25
    for k, case in enumerate(cases):
        x = tc.case_bytes(case, kind, noise[k:])
        y = tc.split_expected(case, x)
        offs, so, do = tc.offsets_of(case), case["src_offset"], case["dst_offset"]
        got = run(ctx, False, x, offs, case["widths"], case["preds"], so, do)
        bad = np.flatnonzero(got != y)
        assert len(bad) == 0, ("split", case["name"], kind, so, do, bad[:8])
        back = run(ctx, True, y, offs, case["widths"], case["preds"], do, so)
        bad = np.flatnonzero(back != x)
        assert len(bad) == 0, ("join", case["name"], kind, do, so, bad[:8])


def test_items_inside_a_larger_buffer_and_no_predictor_table(ctx, noise):
    """The offsets need not begin at 0 or end with the buffer: exactly [offsets[0], offsets[nitems]) is read and written; preds=None
    is no predictor anywhere."""
    n = 20_000
    x = noise[5: 5 + n]
    offs = np.array([777, 777 + 4 * 1000 + 3, 9000, 9000, 15_001], np.uint64)
    widths = np.array([4, 2, 8, 1], np.uint8)
    for preds in (None, np.array([2, 1, 0, 0], np.uint8)):
        want = typed_items.split_numpy(x, offs, widths, preds)
        src, dst = Guarded(n, 3, x, salt=1), Guarded(n, 1, salt=2)
        typed_items.split_device(ctx, src.view, offs, widths, preds, dst.view)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        got = dst.view.cpu().numpy()
        assert np.array_equal(got[777:15_001], want[777:15_001])
        dst.tensor[dst.at + 777: dst.at + 15_001] = dst.before[dst.at + 777: dst.at + 15_001]
        dst.check(0, "split dst outside the items")
        src.check(0, "split src")
        mid, out = Guarded(n, 8, want, salt=3), Guarded(n, 15, salt=4)
        typed_items.join_device(ctx, mid.view, offs, widths, preds, out.view)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(out.view.cpu().numpy()[777:15_001], x[777:15_001])
        out.tensor[out.at + 777: out.at + 15_001] = out.before[out.at + 777: out.at + 15_001]
        out.check(0, "join dst outside the items")


@pytest.mark.parametrize("width", pr.WIDTHS)
@pytest.mark.parametrize("pred", (pr.NONE, pr.DELTA, pr.ZIGZAG))
def test_superblock_cut_items_equal_the_block_calls(ctx, noise, width, pred):
    block = 4096
    n = 3 * width * block + 37
    x = noise[11: 11 + n]
    lengths, widths, preds = tc.superblock_items(n, width, block, pred)
    offs = rcx.item_offsets(lengths)
    assert len(lengths) == 4 and int(lengths[-1]) == 37
    want = run_filter(ctx, lambda src, dst: predict.split_device(ctx, src, width, block, pred, dst), "predict split", x, 1, 3)
    assert np.array_equal(want, pr.split_numpy(x, width, block, pred))
    assert np.array_equal(run(ctx, False, x, offs, widths, preds, 1, 3), want)
    back = run_filter(ctx, lambda src, dst: predict.join_device(ctx, src, width, block, pred, dst), "predict join", want, 3, 1)
    assert np.array_equal(run(ctx, True, want, offs, widths, preds, 3, 1), back) and np.array_equal(back, x)


# ---- many items, and grids that loop -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(noise):
    """65 537 items of 0 to 40 bytes, classes in turn; the expectation once: a batch of fewer items is a prefix of it."""
    rs = np.random.RandomState(65)
    classes = [(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)]
    lengths = rs.randint(0, 41, 65537).astype(np.uint64)
    pick = rs.randint(0, len(classes), 65537)
    widths = np.array([classes[k][0] for k in pick], np.uint8)
    preds = np.array([classes[k][1] for k in pick], np.uint8)
    offs = rcx.item_offsets(lengths)
    x = noise[: int(offs[-1])]
    return lengths, widths, preds, offs, x, typed_items.split_numpy(x, offs, widths, preds)


@pytest.mark.parametrize("nitems", (65535, 65536, 65537))
def test_item_counts_around_two_to_the_sixteen(ctx, many, nitems):
    lengths, widths, preds, offs, x, y = many
    n = int(offs[nitems])
    got = run(ctx, False, x[:n], offs[: nitems + 1], widths[:nitems], preds[:nitems], 1, 8)
    assert np.array_equal(got, y[:n])
    assert np.array_equal(run(ctx, True, y[:n], offs[: nitems + 1], widths[:nitems], preds[:nitems], 3, 0), x[:n])


def test_eight_mebibytes_and_five_bytes(ctx, noise):
    """Items of 0 bytes to a MiB and a tail, every width, side by side: 128 workgroup steps spread over seven classes."""
    n = (8 << 20) + 5
    sizes = [(1 << 20) + 3, 65536, 4 * 4099, 100_000, 8 * 65536 + 7, 33, 2 * 70_000 + 1, 0, 12_345]
    classes = [(8, pr.DELTA), (2, pr.NONE), (4, pr.ZIGZAG), (1, pr.NONE), (8, pr.NONE), (2, pr.ZIGZAG), (4, pr.DELTA)]
    items, total, k = [], 0, 0
    while total < n:
        size = min(sizes[k % len(sizes)], n - total)
        items.append((size, *classes[k % len(classes)]))
        total += size
        k += 1
    lengths = np.array([it[0] for it in items], np.uint64)
    widths, preds = np.array([it[1] for it in items], np.uint8), np.array([it[2] for it in items], np.uint8)
    offs = rcx.item_offsets(lengths)
    x = noise[3: 3 + n]
    y = typed_items.split_numpy(x, offs, widths, preds)
    assert np.array_equal(run(ctx, False, x, offs, widths, preds), y)
    assert np.array_equal(run(ctx, True, y, offs, widths, preds), x)


def test_more_steps_than_the_grid_has_workgroups(ctx, noise):
    """The fixed grid is four workgroups a compute unit (read from the device) and a step is 64 KiB: with 37 steps more than that
    the step loop goes round, in split and in the join without a predictor.  (The rest loop goes round in the test above.)"""
    steps = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    lengths = np.array([3 * 65536 + 2 * 7 + 1] * (steps // 3) + [65536 * (steps % 3) + 2], np.uint64)  # three steps and 7 elements and a byte each
    widths = np.full(len(lengths), 2, np.uint8)
    offs = rcx.item_offsets(lengths)
    n = int(offs[-1])
    x = np.resize(noise, n)
    y = typed_items.split_numpy(x, offs, widths, None)
    assert np.array_equal(run(ctx, False, x, offs, widths, None, 1, 0), y)
    assert np.array_equal(run(ctx, True, y, offs, widths, None, 0, 3), x)


def test_host_buffer_calls(ctx, noise, cases):
    for case in (cases[10], cases[12], cases[15], cases[13]):  # mixed small, empty runs, large and small, only empty
        x = tc.case_bytes(case, "random", noise)
        offs = tc.offsets_of(case)
        y = typed_items.split(ctx, x, offs, case["widths"], case["preds"])
        assert y == tc.split_expected(case, x).tobytes(), case["name"]
        assert typed_items.join(ctx, y, offs, case["widths"], case["preds"]) == x.tobytes(), case["name"]
    x = noise[:3000]
    offs, widths = np.array([100, 1100, 2103], np.uint64), np.array([8, 2], np.uint8)  # the copy begins at the first item
    y = typed_items.split(ctx, x, offs, widths, [1, 2])
    assert y == typed_items.split_numpy(x, offs, widths, [1, 2]).tobytes() and typed_items.join(ctx, y, offs, widths, [1, 2]) == x.tobytes()


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(ctx, noise):
    L, h = typed_items.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    src, dst = Guarded(n, 0, noise[:n], salt=1), Guarded(n, 0, salt=2)
    room = Guarded(3 * n, 0, noise[: 3 * n], salt=3)  # one allocation for the overlapping and the adjacent ranges
    s, d, r = src.view.data_ptr(), dst.view.data_ptr(), room.view.data_ptr()
    host_out = np.full(n, 0xA5, np.uint8)

    def tables(offs, widths, preds=None):
        t = (np.array(offs, np.uint64), np.array(widths, np.uint8), None if preds is None else np.array(preds, np.uint8))
        return t, (t[0].ctypes.data, t[1].ctypes.data, None if t[2] is None else t[2].ctypes.data, len(widths))

    good, g = tables([0, 1000, n], [4, 2], [1, 0])
    big = (1 << 24) - 256
    bad_tables = [tables([0, 1000, n], [4, 3]), tables([0, 1000, n], [0, 2]), tables([0, 1000, n], [4, 16]),           # a width
                  tables([0, 1000, n], [4, 2], [3, 0]), tables([0, 1000, n], [4, 2], [0, 255]),                          # a predictor
                  tables([0, 1000, n], [1, 2], [1, 0]), tables([0, 1000, n], [4, 1], [0, 2]),                            # ... with width 1
                  tables([0, 1000, 999], [4, 2]), tables([n, 0], [2]),                                                  # decreasing offsets
                  tables([0, 8 * (big + 1)], [8]), tables([0, big + 1], [1]), tables([0, 2 * big + 2], [2]),            # a sub-item above the limit
                  tables([0, 0, 0], [4, 3]), tables([0, 0], [1], [1])]                                                  # ... also with nothing to do
    for fn in (L.rcx_typed_items_split_device, L.rcx_typed_items_join_device):
        assert fn(h, s, None, None, None, 0, d, stream) == rcx.OK and fn(h, None, None, None, None, 0, None, stream) == rcx.OK  # nitems = 0
        empty, e = tables([5, 5, 5], [2, 1], [2, 0])
        assert fn(h, None, *e, None, stream) == rcx.OK and fn(h, s, *e, d, stream) == rcx.OK                                       # no bytes
        for keep, t in bad_tables:
            assert fn(h, s, *t, d, stream) == rcx.E_ARG, keep
        for st in (fn(None, s, *g, d, stream), fn(h, None, *g, d, stream), fn(h, s, *g, None, stream),                            # null pointers
                   fn(h, s, None, g[1], g[2], 2, d, stream), fn(h, s, g[0], None, g[2], 2, d, stream),                            # null tables
                   fn(h, r, *g, r, stream), fn(h, r, *g, r + 1, stream), fn(h, r + 1, *g, r, stream),                              # overlaps
                   fn(h, r, *g, r + n - 1, stream), fn(h, r + n - 1, *g, r, stream)):
            assert st == rcx.E_ARG
    for fn in (L.rcx_typed_items_split, L.rcx_typed_items_join):
        for keep, t in bad_tables:
            assert fn(h, noise.ctypes.data, *t, host_out.ctypes.data) == rcx.E_ARG, keep
        for st in (fn(h, None, *g, host_out.ctypes.data), fn(h, noise.ctypes.data, *g, None), fn(h, noise.ctypes.data, *g, noise.ctypes.data + 100),
                   fn(None, noise.ctypes.data, *g, host_out.ctypes.data)):
            assert st == rcx.E_ARG
        assert fn(h, None, None, None, None, 0, None) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for buf, what in ((src, "src"), (dst, "dst"), (room, "room")):
        buf.check(0, what)  # not a byte changed anywhere
    assert bool((host_out == 0xA5).all())
    # ranges that touch are apart: the second third of the allocation from its first, and the third from the second
    y = typed_items.split_numpy(noise[:n], *good)
    assert L.rcx_typed_items_split_device(h, r, *g, r + n, stream) == rcx.OK
    assert L.rcx_typed_items_join_device(h, r + n, *g, r + 2 * n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[:n], noise[:n]) and np.array_equal(got[n: 2 * n], y) and np.array_equal(got[2 * n:], noise[:n])
    room.check(3 * n, "room")


# ---- containers ------------------------------------------------------------------------------------------------------------------
def container_items():
    """(bytes, width, predictor by name): sorted keys, floats, plain bytes, a random walk with a tail, nothing, less than an element,
    indices."""
    torch.manual_seed(3)
    return [(pr.integer_bytes("sorted_keys", 1 << 16)[0][: 8 * 1000 + 5], 8, "delta"),
            ((torch.randn(2500) * 0.02).to(torch.bfloat16).view(torch.uint8).numpy().copy(), 2, None),
            (np.frombuffer(b"plain bytes, thirty-three of them", np.uint8), 1, None),
            (pr.integer_bytes("random_walk", 1 << 16)[0][: 4 * 3000 + 3], 4, "zigzag"),
            (np.zeros(0, np.uint8), 4, "delta"),
            (np.arange(7, dtype=np.uint8), 8, "zigzag"),
            (pc.index_bytes(1 << 14)[0], 8, None)]


@pytest.fixture(scope="module")
def packed_sub_items():
    """The items, their tables, the split text and its sub-items (numpy)."""
    items = container_items()
    parts = [it[0] for it in items]
    widths = np.array([it[1] for it in items], np.uint8)
    preds = np.array([container.PREDICTORS[it[2]] for it in items], np.uint8)
    offs = rcx.item_offsets([len(x) for x in parts])
    y = typed_items.split_numpy(np.concatenate(parts), offs, widths, preds)
    sub = typed_items.sub_offsets_numpy(offs, widths)
    return items, widths, preds, y, sub, [y[int(sub[k]): int(sub[k + 1])] for k in range(len(sub) - 1)]


@pytest.mark.parametrize("coder", CODERS)
def test_sub_item_streams_are_the_oracles(ctx, oracle, packed_sub_items, coder):
    items, widths, preds, y, sub, subs = packed_sub_items
    want = oracle_streams(oracle, subs, coder)
    for checksum in (False, True):
        blob = container.pack_typed_items([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], coder, ctx, checksum=checksum,
                                          directory=b"carried")
        c = container.parse_typed_items(blob)
        assert (c["coder"], c["nitems"], c["nsub"], c["directory"]) == (coder, len(items), int(widths.sum()), b"carried")
        assert list(c["widths"]) == list(widths) and list(c["preds"]) == list(preds) and list(c["lengths"]) == [len(it[0]) for it in items]
        assert_same_items(c["payload"], c["offsets"], want, (coder, checksum))
        if checksum:
            assert list(c["crcs"]) == [zlib.crc32(s.tobytes()) if len(s) else 0 for s in subs]
        else:
            assert c["crcs"] is None
        assert container.unpack_typed_items(blob, ctx=ctx) == [it[0].tobytes() for it in items]


@pytest.mark.parametrize("checksum", (False, True))
def test_picks(ctx, monkeypatch, checksum):
    items = container_items()
    raw = [it[0].tobytes() for it in items]
    blob = container.pack_typed_items([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], 0, ctx, checksum=checksum)
    c = container.parse_typed_items(blob)
    seen, real = [], ctx.decode_items_device

    def decode_items_device(*a, pick=None, **kw):
        seen.append([int(k) for k in pick])
        return real(*a, pick=pick, **kw)

    monkeypatch.setattr(ctx, "decode_items_device", decode_items_device)
    first = [int(v) for v in c["sub_first"]]
    for pick in ([0], [3, 0], [6, 5, 4, 3, 2, 1, 0], [1, 1, 3, 1], [2], [2, 2], [5], [4, 2, 4]):
        assert container.unpack_typed_items(blob, pick, ctx) == [raw[k] for k in pick], pick
        assert seen[-1] == [s for k in pick for s in range(first[k], first[k + 1])], pick  # the picks' sub-items and no others
    calls = len(seen)
    assert container.unpack_typed_items(blob, [], ctx) == [] and container.unpack_typed_items(blob, [4], ctx) == [b""] and len(seen) == calls
    assert container.unpack_typed_items(blob, None, ctx) == raw and container.unpack_typed_items(blob, ctx=ctx, verify=False) == raw
    with pytest.raises(container.ContainerError):
        container.unpack_typed_items(blob, [7], ctx)


def test_auto_writes_the_container_of_its_picks(ctx):
    keys = pr.integer_bytes("sorted_keys", 1 << 17)[0]
    walk = pr.integer_bytes("random_walk", 1 << 17)[0]
    floats = pc.randn_bytes("bf16", 1 << 16)[0]
    index = pc.index_bytes(1 << 16)[0]
    items = [keys[:40_000], floats, walk[: 4 * 9000 + 2], index, np.arange(200, dtype=np.uint8), keys[40_000:40_000 + 8 * 2048], np.zeros(0, np.uint8), walk[:3]]
    widths = [8, 2, 4, 8, 1, 8, 4, 4]
    for checksum in (False, True):
        auto = container.pack_typed_items(items, widths, "auto", 0, ctx, checksum=checksum)
        c = container.parse_typed_items(auto)
        names = [{0: None, 1: "delta", 2: "zigzag"}[int(p)] for p in c["preds"]]
        assert names == ["delta", None, "zigzag", None, None, "delta", None, None], names
        assert container.pack_typed_items(items, widths, names, 0, ctx, checksum=checksum) == auto
        assert container.unpack_typed_items(auto, ctx=ctx) == [x.tobytes() for x in items]
    # a list may mix names and "auto"
    mixed = container.pack_typed_items(items, widths, ["zigzag", "auto", "auto", None, None, "auto", "auto", "delta"], 0, ctx)
    assert list(container.parse_typed_items(mixed)["preds"]) == [2, 0, 2, 0, 0, 1, 0, 1]


def silent_flip(oracle, stream, good):
    """A single-bit flip near the end of `stream` that the oracle decodes completely, to other bytes -> (byte, bit)."""
    for back in range(6, 70):
        for bit in (0x01, 0x10, 0x80):
            s = stream.copy()
            s[len(s) - back] ^= bit
            ok, out = oracle_decode_one(oracle, s, len(good), 0, max(len(good), 16))
            if ok and not np.array_equal(out, good):
                return len(s) - back, bit
    return None


def test_a_flipped_payload_byte_names_its_item(ctx, oracle, packed_sub_items):
    items, widths, preds, y, sub, subs = packed_sub_items
    raw = [it[0].tobytes() for it in items]
    blob = container.pack_typed_items([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], 0, ctx, checksum=True)
    c = container.parse_typed_items(blob)
    payload_at = len(blob) - len(c["payload"])
    for item, plane in ((3, 0), (0, 1), (6, 0)):
        k = int(c["sub_first"][item]) + plane
        stream = np.array(c["payload"][int(c["offsets"][k]): int(c["offsets"][k + 1])])
        at = silent_flip(oracle, stream, subs[k])
        assert at is not None, "no flip that the oracle decodes to other bytes"
        bad = bytearray(blob)
        bad[payload_at + int(c["offsets"][k]) + at[0]] ^= at[1]
        bad = bytes(bad)
        with pytest.raises(container.ChecksumError) as e:
            container.unpack_typed_items(bad, ctx=ctx)
        assert (e.value.kind, e.value.index) == ("item", item)
        with pytest.raises(container.ChecksumError) as e:
            container.unpack_typed_items(bad, [1, item, 2], ctx)
        assert e.value.index == item  # the container's item, not its place among the picks
        others = [j for j in range(len(items)) if j != item]
        assert container.unpack_typed_items(bad, others, ctx) == [raw[j] for j in others]  # an item that was not picked is not checked
        got = container.unpack_typed_items(bad, ctx=ctx, verify=False)  # nobody asked: the bytes as they decode, damage inside its item
        assert got[item] != raw[item] and len(got[item]) == len(raw[item]) and [got[j] for j in others] == [raw[j] for j in others]
    assert container.unpack_typed_items(blob, ctx=ctx) == raw


# ---- tensors with names --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", pr.WIDTHS)
def test_one_tensor_carries_the_payload_of_pack_typed(ctx, width):
    block = 4096
    dtype = {2: torch.int16, 4: torch.int32, 8: torch.int64}[width]
    torch.manual_seed(width)
    t = torch.cumsum(torch.randint(-50, 51, (3 * block,)), 0).to(dtype)
    assert t.numel() * t.element_size() == 3 * width * block
    for predict_, checksum in ((None, False), ("zigzag", True)):
        typed = container.parse_typed(container.pack_typed(t, None, block, 0, ctx, checksum=checksum, predict=predict_))
        blob = container.pack_tensors({"t": t}, block=block, predict=predict_, ctx=ctx, checksum=checksum)
        c = container.parse_typed_items(blob)
        assert c["nitems"] == 3 and c["nsub"] == typed["nblocks"] == 3 * width and list(c["lengths"]) == [width * block] * 3
        assert np.array_equal(c["payload"], typed["payload"]) and np.array_equal(c["offsets"], typed["offsets"])  # the same streams back to back
        if checksum:
            assert np.array_equal(c["crcs"], typed["crcs"])
        assert torch.equal(container.unpack_tensors(blob, ctx=ctx)["t"], t)


def state_dict():
    torch.manual_seed(11)
    return {"layer.weight": (torch.randn(300, 70) * 0.02).to(torch.bfloat16), "layer.norm": torch.randn(1000) * 0.02 + 1,
            "table": torch.sort(torch.randint(0, 10 ** 9, (5000,)))[0], "mask": torch.rand(4099) < 0.2,
            "bytes": torch.randint(0, 256, (3, 1000), dtype=torch.uint8), "empty": torch.zeros(0, 4, dtype=torch.float32),
            "scalar": torch.tensor(3.25, dtype=torch.float32), "five": torch.arange(5, dtype=torch.uint8), "half": torch.randn(17, dtype=torch.float16)}


@pytest.mark.parametrize("source", ("cpu", "cuda", "numpy"))
@pytest.mark.parametrize("device", ("cpu", "cuda"))
def test_a_state_dict_round_trips(ctx, source, device):
    named = state_dict()
    want = container.pack_tensors(named, block=4096, predict="auto", ctx=ctx, checksum=True)
    given = {k: v.cuda() for k, v in named.items()} if source == "cuda" else \
        {k: (v.numpy() if v.dtype != torch.bfloat16 else v) for k, v in named.items()} if source == "numpy" else named
    blob = container.pack_tensors(given, block=4096, predict="auto", ctx=ctx, checksum=True)
    assert blob == want  # where the bytes lie changes nothing
    c = container.parse_typed_items(blob)
    entries = container.parse_tensor_directory(c["directory"], c["nitems"])
    assert [e["name"] for e in entries] == list(named) and [e["dtype"] for e in entries] == [str(v.dtype).replace("torch.", "") for v in named.values()]
    assert [e["count"] for e in entries] == [-(-v.numel() * v.element_size() // (v.element_size() * 4096)) for v in named.values()]
    by_name = {e["name"]: e for e in entries}
    table = by_name["table"]
    assert set(c["preds"][table["first"]: table["first"] + table["count"]]) == {1} and not c["preds"][c["widths"] == 1].any()  # sorted keys take delta
    back = container.unpack_tensors(blob, device=device, ctx=ctx)
    assert list(back) == list(named)
    for name, t in named.items():
        assert back[name].device.type == device and back[name].dtype == t.dtype and back[name].shape == t.shape, name
        assert torch.equal(back[name].cpu(), t), name


def test_names_decode_only_their_items(ctx, monkeypatch):
    named = state_dict()
    blob = container.pack_tensors(named, block=4096, ctx=ctx, checksum=True)
    c = container.parse_typed_items(blob)
    by_name = {e["name"]: e for e in container.parse_tensor_directory(c["directory"], c["nitems"])}
    seen, real = [], ctx.decode_items_device

    def decode_items_device(*a, pick=None, **kw):
        seen.append(len(pick))
        return real(*a, pick=pick, **kw)

    monkeypatch.setattr(ctx, "decode_items_device", decode_items_device)
    for names in (["table"], ["five", "layer.weight"], ["scalar", "empty"], ["mask"]):
        back = container.unpack_tensors(blob, names=names, ctx=ctx)
        assert list(back) == names and all(torch.equal(back[n], named[n]) for n in names)
        assert seen[-1] == sum(by_name[n]["count"] * named[n].element_size() for n in names), names  # streams handed to the decode call
    calls = len(seen)
    assert list(container.unpack_tensors(blob, names=["empty"], ctx=ctx)) == ["empty"] and len(seen) == calls  # nothing to decode
    with pytest.raises(container.ContainerError):
        container.unpack_tensors(blob, names=["nobody"], ctx=ctx)
