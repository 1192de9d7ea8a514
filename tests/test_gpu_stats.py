"""Byte counts and order-0 costs per block and item on the GPU (include/rcx_stats.h) against np.bincount and
stats.cost_numpy, exactly; and pack_typed(predict="auto"), which decides by them.

The kernel (csrc/rcx_stats.hpp) gives an entry of at most 1024 bytes to one wave, four to a workgroup, and a longer one to
the whole workgroup, 16 bytes a thread and four such loads in flight; a fixed grid loops.  The shapes of stats_cases
cover both kinds of entry, their border, entries off the 16-byte pieces, the rows of loads, and grids that loop; the data
covers what the merge of equal neighbours meets: no runs, one run, runs of one, runs cut by the 16-byte pieces.  (predict_cases.looping_cases is sized
for the inverse predictor's waves and widths, which mean nothing here: the looping shapes are made from this grid's own size.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import predict_cases as pr
import stats_cases as sc
from cpprcoder_amd import container, rcx, stats
from gpu_support import Guarded, ctx, knobs  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise():
    """RCX_MAX_BLOCK random bytes and a MiB more: every case below is a slice of them."""
    return np.random.RandomState(20251).randint(0, 256, rcx.MAX_BLOCK + (1 << 20), dtype=np.uint8)


class Tables:
    """Guarded room for `count` rows of counts and as many costs; either may be withheld from the call."""

    def __init__(self, count):
        self.count = count
        self.hist = Guarded(1024 * count, salt=7)
        self.cost = Guarded(8 * count, salt=8)
        assert self.hist.view.data_ptr() % 4 == 0 and self.cost.view.data_ptr() % 8 == 0

    def d_hist(self):
        return self.hist.view.view(torch.int32)

    def d_cost(self):
        return self.cost.view.view(torch.int64)

    def read(self, hist=True, cost=True):
        """-> (counts uint32 [count, 256], costs uint64 [count]) after checking that nothing else changed: of a table that
        was withheld not one byte."""
        self.hist.check(1024 * self.count if hist else 0, "d_hist")
        self.cost.check(8 * self.count if cost else 0, "d_cost")
        return (self.hist.view.cpu().numpy().view(np.uint32).reshape(self.count, 256).copy(),
                self.cost.view.cpu().numpy().view(np.uint64).copy())


def blocks_on_gpu(ctx, x, block, offset=0, hist=True, cost=True):
    src = Guarded(len(x), offset, x, salt=1)
    assert src.view.data_ptr() % 16 == offset % 16
    t = Tables(rcx.block_count(len(x), block))
    stats.blocks_device(ctx, src.view, block, t.d_hist() if hist else None, t.d_cost() if cost else None)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    src.check(0, "src")
    return t.read(hist, cost)


def items_on_gpu(ctx, x, offs, offset=0, hist=True, cost=True):
    src = Guarded(len(x), offset, x, salt=1)
    t = Tables(len(offs) - 1)
    stats.items_device(ctx, src.view, offs, t.d_hist() if hist else None, t.d_cost() if cost else None)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    src.check(0, "src")
    return t.read(hist, cost)


def assert_tables(got, want_hist, label):
    hist, cost = got
    bad = np.flatnonzero((hist != want_hist).any(axis=1))
    assert len(bad) == 0, (label, "counts of entry", bad[:8])
    want_cost = stats.cost_numpy(want_hist)
    bad = np.flatnonzero(cost != want_cost)
    assert len(bad) == 0, (label, "cost of entry", bad[:8], cost[bad[:4]], want_cost[bad[:4]])


# ---- parity with numpy: blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", sc.BLOCKS)
def test_blocks_against_numpy(ctx, noise, block):
    for k, n in enumerate(sc.sizes(block)):
        for j, kind in enumerate(sc.KINDS):
            x = sc.data(kind, n, noise)
            offset = sc.OFFSETS[(k + j) % 5]  # five sizes, four kinds: every block size meets every offset
            assert_tables(blocks_on_gpu(ctx, x, block, offset), sc.hist_blocks(x, block), (block, n, kind, offset))


def test_the_ends_of_the_cost(ctx):
    one = np.full(3 * 4096, 9, np.uint8)
    hist, cost = blocks_on_gpu(ctx, one, 4096)
    assert [int(v) for v in cost] == [0, 0, 0] and bool((hist[:, 9] == 4096).all()) and int(hist.sum()) == 3 * 4096
    flat = sc.data("each_once", 2 * 65536, None)
    hist, cost = blocks_on_gpu(ctx, flat, 65536)
    assert bool((hist == 256).all()) and [int(v) for v in cost] == [65536 * 8 * 65536] * 2


def test_counts_around_two_to_the_sixteen(ctx, noise):
    """Blocks of 66000 bytes in which one symbol occurs 65535, 65536 and 65537 times, scattered; the others share the rest."""
    block, parts = 66000, []
    rs = np.random.RandomState(65536)
    for count in (65535, 65536, 65537):
        b = (noise[: block] % 255).astype(np.uint8)  # 0 .. 254
        b[rs.permutation(block)[:count]] = 255
        parts.append(b)
    x = np.concatenate(parts)
    want = sc.hist_blocks(x, block)
    assert [int(v) for v in want[:, 255]] == [65535, 65536, 65537]
    assert_tables(blocks_on_gpu(ctx, x, block, 3), want, "2^16")
    # and in runs: the merge adds up to 16 at once
    x = np.sort(x.reshape(3, block), axis=1).reshape(-1)
    assert_tables(blocks_on_gpu(ctx, x, block, 1), sc.hist_blocks(x, block), "2^16, sorted")


def test_grids_that_loop(ctx, noise):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    most = 8 * cus  # csrc/rcx_stats_api.hpp stats_launch: workgroups in the fixed grid
    for block, count in ((16, 4 * (most + most // 2) + 3), (1040, most + most // 2 + 1)):  # four short entries a workgroup, one long
        n = count * block + block // 2 + 1
        assert n <= len(noise)
        x = noise[:n]
        assert_tables(blocks_on_gpu(ctx, x, block, 1), sc.hist_blocks(x, block), (block, n))


def test_host_calls_and_one_entry_launches(ctx, noise):
    for n, block in ((1, 16), (16, 16), (1000, 4096), (65536, 65536), (rcx.MAX_BLOCK, rcx.MAX_BLOCK)):
        x = noise[7: 7 + n]
        want = sc.hist_blocks(x, block)
        assert len(want) == 1
        assert_tables(blocks_on_gpu(ctx, x, block, 8), want, (n, block))
        assert_tables(stats.blocks(ctx, x, block), want, ("host", n, block))
        assert_tables(items_on_gpu(ctx, x, np.array([0, n], np.uint64), 15), want, ("one item", n))
    x = noise[: 5 * 4096 + 99]
    assert_tables(stats.blocks(ctx, x.tobytes(), 4096), sc.hist_blocks(x, 4096), "host blocks")
    hist, cost = stats.blocks(ctx, b"", 4096)
    assert hist.shape == (0, 256) and cost.shape == (0,)


# ---- parity with numpy: items -------------------------------------------------------------------------------------------------
def test_items_of_every_kind_in_one_call(ctx, noise):
    rs = np.random.RandomState(9)
    lengths = np.array([0, 1, 15, 16, 17, 4 << 20, 0, sc.SHORT - 1, sc.SHORT, sc.SHORT + 1, sc.SHORT + 16, 4096, 70_001] + [64] * 300)
    lengths = lengths[rs.permutation(len(lengths))]
    offs = rcx.item_offsets(lengths)
    x = noise[5: 5 + int(offs[-1])].copy()
    x[int(offs[20]): int(offs[21])] = 0x33  # one item of one repeated byte
    want = sc.hist_items(x, offs)
    assert int(want[np.flatnonzero(lengths == 0)].sum()) == 0
    for offset in (0, 3):
        got = items_on_gpu(ctx, x, offs, offset)
        assert_tables(got, want, ("items", offset))
        assert [int(v) for v in got[1][lengths == 0]] == [0, 0]  # an empty item: cost 0 and a row of zeros
    assert_tables(stats.items(ctx, x, lengths), want, "host items")
    parts = [x[int(offs[i]): int(offs[i + 1])] for i in range(40)]
    assert_tables(stats.items(ctx, parts), want[:40], "host items, a list")
    # the caller's order (diagnostic): every entry is taken as a long one
    with knobs({"RCX_ITEMS_ORDER": "0"}):
        assert_tables(items_on_gpu(ctx, x, offs, 1), want, "items in the caller's order")
    # only short ones, and only empty ones
    offs = rcx.item_offsets([64] * 9 + [0] + [17] * 3)
    assert_tables(items_on_gpu(ctx, noise[: int(offs[-1])], offs, 15), sc.hist_items(noise, offs), "short items")
    hist, cost = stats.items(ctx, [b"", b""])
    assert int(hist.sum()) == 0 and [int(v) for v in cost] == [0, 0]
    hist, cost = stats.items(ctx, [])
    assert hist.shape == (0, 256) and len(cost) == 0


# ---- output selection and refusals ---------------------------------------------------------------------------------------------
def test_either_table_alone(ctx, noise):
    x = noise[: 3 * 4096 + 700]
    want = sc.hist_blocks(x, 4096)
    hist, _ = blocks_on_gpu(ctx, x, 4096, 1, cost=False)  # (Tables.read: not one byte of the table withheld changed)
    assert np.array_equal(hist, want)
    _, cost = blocks_on_gpu(ctx, x, 4096, 1, hist=False)
    assert np.array_equal(cost, stats.cost_numpy(want))
    offs = rcx.item_offsets([100, 0, 3000, 64])
    hist, _ = items_on_gpu(ctx, x, offs, cost=False)
    assert np.array_equal(hist, sc.hist_items(x, offs))
    _, cost = items_on_gpu(ctx, x, offs, hist=False)
    assert np.array_equal(cost, stats.cost_numpy(sc.hist_items(x, offs)))


def test_nothing_to_do_and_bad_arguments_write_nothing(ctx, noise):
    L, h = stats.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    src_g = Guarded(3 * 4096, 0, noise[: 3 * 4096], salt=1)
    t = Tables(8)
    offs = rcx.item_offsets([100, 200, 300])
    src, hist, cost, o = src_g.view.data_ptr(), t.d_hist().data_ptr(), t.d_cost().data_ptr(), offs.ctypes.data
    # nothing to do
    assert L.rcx_stats_blocks_device(h, src, 0, 4096, hist, cost, stream) == rcx.OK
    assert L.rcx_stats_blocks_device(h, None, 0, 4096, None, None, stream) == rcx.OK
    assert L.rcx_stats_items_device(h, src, o, 0, hist, cost, stream) == rcx.OK
    assert L.rcx_stats_items_device(h, None, None, 0, None, None, stream) == rcx.OK
    assert L.rcx_stats_blocks(h, None, 0, 4096, None, None) == rcx.OK and L.rcx_stats_items(h, None, None, 0, None, None) == rcx.OK
    # RCX_E_ARG before anything is enqueued
    down = np.array([0, 100, 50, 300], np.uint64)
    long = np.array([0, rcx.MAX_BLOCK + 1], np.uint64)
    n = 3 * 4096
    host = noise.ctypes.data
    h_hist, h_cost = np.zeros((8, 256), np.uint32), np.zeros(8, np.uint64)
    for st in (L.rcx_stats_blocks_device(h, src, n, 15, hist, cost, stream), L.rcx_stats_blocks_device(h, src, n, 0, hist, cost, stream),
               L.rcx_stats_blocks_device(h, src, n, rcx.MAX_BLOCK + 1, hist, cost, stream),
               L.rcx_stats_blocks_device(h, None, n, 4096, hist, cost, stream), L.rcx_stats_blocks_device(h, src, n, 4096, None, None, stream),
               L.rcx_stats_blocks_device(None, src, n, 4096, hist, cost, stream),
               # an output inside the source: its first byte, its last, and a table that begins in front of it and runs into it
               L.rcx_stats_blocks_device(h, src, n, 4096, src, cost, stream), L.rcx_stats_blocks_device(h, src, n, 4096, hist, src + n - 8, stream),
               L.rcx_stats_blocks_device(h, src, n, 4096, src - 3 * 1024 + 4, None, stream), L.rcx_stats_blocks_device(h, src, n, 4096, None, src - 16, stream),
               L.rcx_stats_items_device(h, None, o, 3, hist, cost, stream), L.rcx_stats_items_device(h, src, None, 3, hist, cost, stream),
               L.rcx_stats_items_device(h, src, o, 3, None, None, stream), L.rcx_stats_items_device(h, src, down.ctypes.data, 3, hist, cost, stream),
               L.rcx_stats_items_device(h, src, long.ctypes.data, 1, hist, cost, stream), L.rcx_stats_items_device(h, src, o, 3, src + 596, cost, stream),
               L.rcx_stats_items_device(h, src, o, 3, hist, src, stream), L.rcx_stats_items_device(None, src, o, 3, hist, cost, stream),
               L.rcx_stats_blocks(h, None, n, 4096, h_hist.ctypes.data, h_cost.ctypes.data), L.rcx_stats_blocks(h, host, n, 15, h_hist.ctypes.data, h_cost.ctypes.data),
               L.rcx_stats_blocks(h, host, n, 4096, None, None), L.rcx_stats_items(h, host, down.ctypes.data, 3, h_hist.ctypes.data, h_cost.ctypes.data),
               L.rcx_stats_items(h, None, o, 3, h_hist.ctypes.data, h_cost.ctypes.data), L.rcx_stats_items(h, host, o, 3, None, None),
               L.rcx_stats_items(h, host, long.ctypes.data, 1, h_hist.ctypes.data, h_cost.ctypes.data)):
        assert st == rcx.E_ARG
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    torch.cuda.synchronize()
    t.read(hist=False, cost=False)  # not one byte of either table changed, nor anything around them
    src_g.check(0, "src")
    assert int(h_hist.sum()) == 0 and int(h_cost.sum()) == 0
    # the binding refuses a table that is too small; and the context still works
    with pytest.raises(ValueError):
        stats.blocks_device(ctx, src_g.view, 4096, t.d_hist()[: 256 * 2], None)
    assert_tables(blocks_on_gpu(ctx, noise[:n], 4096), sc.hist_blocks(noise[:n], 4096), "after the refusals")


def test_needs_no_reserve_and_takes_any_stream(noise):
    fresh = rcx.Context(0)
    try:
        x = noise[: 9 * 4096 + 5]
        d_src = torch.from_numpy(x).cuda()
        t = Tables(10)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        stats.blocks_device(fresh, d_src, 4096, t.d_hist(), t.d_cost(), stream=side)
        assert fresh.sync_status(stream=side, raise_on_error=False)[0] == rcx.OK
        side.synchronize()
        assert_tables(t.read(), sc.hist_blocks(x, 4096), "side stream")
        assert fresh.scratch_bytes() == 0  # nothing was allocated for it
    finally:
        fresh.close()


# ---- capture -------------------------------------------------------------------------------------------------------------------
def test_one_launch_replays_from_a_graph(ctx, noise):
    """One captured launch, no branches; replayed twice, the second time on other bytes."""
    block, n = 4096, 6 * 4096 + 123
    first, second = noise[:n], noise[n: 2 * n]
    d_src = torch.from_numpy(first.copy()).cuda()
    t = Tables(7)
    d_hist, d_cost = t.d_hist(), t.d_cost()
    stats.blocks_device(ctx, d_src, block, d_hist, d_cost)  # once outside, so that nothing happens for the first time in the capture
    torch.cuda.synchronize()
    assert_tables(t.read(), sc.hist_blocks(first, block), "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stats.blocks_device(ctx, d_src, block, d_hist, d_cost)
    for x in (first, second):
        d_src.copy_(torch.from_numpy(x.copy()).cuda())
        t.hist.view.zero_()
        t.cost.view.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_tables(t.read(), sc.hist_blocks(x, block), "replay")
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK


# ---- the consumer: pack_typed(predict="auto") ------------------------------------------------------------------------------------
AUTO_N, AUTO_BLOCK = 256 << 10, 4096


@pytest.mark.parametrize("name", tuple(sc.PICKS))
def test_auto_is_the_rule_on_the_measured_costs(ctx, name):
    x, width = sc.typed_bytes(name)
    x = x[:AUTO_N]
    costs = sc.split_costs(x, width, AUTO_BLOCK)
    pick = container.pick_predictor(*costs)
    print(name, [sc.cost_bytes(c) for c in costs], pick)
    # the sums the decision is taken on are the mirror's
    for pred, want in zip((pr.NONE, pr.DELTA, pr.ZIGZAG), costs):
        _, cost = stats.blocks(ctx, pr.split_numpy(x, width, AUTO_BLOCK, pred), AUTO_BLOCK)
        assert int(cost.sum(dtype=np.uint64)) == want, (name, pred)
    sources = (torch.from_numpy(x.copy()).cuda().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[width]),
               torch.from_numpy(x.copy()).view({2: torch.int16, 4: torch.int32, 8: torch.int64}[width]), x.tobytes())
    for checksum in (False, True):
        named = container.pack_typed(x.tobytes(), width, AUTO_BLOCK, 0, ctx, checksum=checksum, predict=pick)
        assert named[4] == (2 if pick else 1) and named[29] == container.PREDICTORS[pick]
        for source in sources:
            blob = container.pack_typed(source, width if isinstance(source, bytes) else None, AUTO_BLOCK, 0, ctx, checksum=checksum, predict="auto")
            assert blob == named, (name, checksum, type(source))
        assert container.unpack_typed(named, ctx) == x.tobytes()
        lo, hi = 3 * width * AUTO_BLOCK + 5, 5 * width * AUTO_BLOCK - 9
        assert container.unpack_typed_range(named, lo, hi, ctx) == x[lo:hi].tobytes()
        assert container.unpack_typed_range(named, len(x) - 100, len(x), ctx) == x[-100:].tobytes()
    if name == "random_walk":  # and with another coder and a ragged end
        ragged = x[: 5 * 4 * AUTO_BLOCK + 1234]
        want = container.pick_predictor(*sc.split_costs(ragged, 4, AUTO_BLOCK))
        blob = container.pack_typed(ragged, 4, AUTO_BLOCK, 1, ctx, predict="auto")
        assert blob == container.pack_typed(ragged, 4, AUTO_BLOCK, 1, ctx, predict=want) and container.unpack_typed(blob, ctx) == ragged.tobytes()


def run_cli(*a):
    return subprocess.run([sys.executable, "-m", "cpprcoder_amd", *a], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=600)


def test_cli_names_the_choice(tmp_path):
    keys = sc.typed_bytes("sorted_keys")[0][:AUTO_N]
    (tmp_path / "keys.bin").write_bytes(keys.tobytes())
    (tmp_path / "noise.bin").write_bytes(sc.typed_bytes("uniform")[0][:AUTO_N].tobytes())
    r = run_cli("t", "--planes", "8", "--predict", "auto", "-b", "4096", str(tmp_path / "keys.bin"), str(tmp_path / "noise.bin"))
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    rows = [line for line in r.stdout.splitlines() if ".bin|" in line]
    want = container.pick_predictor(*sc.split_costs(keys, 8, 4096))
    assert len(rows) == 2 and rows[0].endswith(f"predict={want}") and rows[1].endswith("predict=none"), r.stdout
