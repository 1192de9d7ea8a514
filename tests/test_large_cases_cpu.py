"""tests/large_cases.py held to what tests/test_gpu_past_4gib.py relies on, without a GPU: the arithmetic of the periodic buffer,
the condition that the compacted payload passes 2^32 as well (from the oracle on the tile alone), and the checkers -- which
must notice a planted difference and name its period, since a checker that cannot fail is the one way the periodic method
could hide a defect."""
import numpy as np
import pytest

import large_cases as lc
import oracle_lib
import planes_cases
import typed_items_cases
from cpprcoder_amd import workloads

torch = pytest.importorskip("torch")


def test_where_the_borders_fall():
    assert lc.T == 8 << 20 == 1 << 23 and lc.K == 513 and lc.TAIL == 12345 and lc.N == 513 * (1 << 23) + 12345 == 4_303_368_249
    assert 256 * lc.T == 1 << 31                      # period 256 begins at 2^31
    assert 512 * lc.T == 1 << 32 and lc.K - 1 == 512  # period 512, the last, begins at exactly 2^32: wholly past it
    assert lc.N > 1 << 32 and lc.N - lc.K * lc.T == lc.TAIL
    # the tile is a whole number of every unit used: blocks, block-sort blocks, superblocks of every width
    assert lc.T % lc.BLOCK == 0 and lc.T // lc.BLOCK == 128 == lc.BLOCKS_PER_TILE
    assert lc.T % oracle_lib.BWT_BLOCK == 0 and lc.T // oracle_lib.BWT_BLOCK == 256
    for w in planes_cases.WIDTHS:
        assert lc.T % (w * lc.BLOCK) == 0
    assert lc.T // (8 * lc.BLOCK) == 16
    # the tail: a short last block, and tail bytes for every width (it is odd)
    assert 0 < lc.TAIL < oracle_lib.BWT_BLOCK < lc.BLOCK and lc.TAIL % 2 == 1
    assert [lc.TAIL % w for w in (2, 4, 8)] == [1, 1, 1]
    assert lc.NBLOCKS == -(-lc.N // lc.BLOCK) == 65665 and lc.NBLOCKS > 65536
    # the block that holds byte 2^32 is the first of period 512
    assert (1 << 32) // lc.BLOCK == 512 * lc.BLOCKS_PER_TILE == 65536


def test_the_tiles():
    x = lc.tile("coder")
    assert x.dtype == np.uint8 and len(x) == lc.T and not x.flags.writeable and lc.tile("coder") is x
    plain = workloads.uniform(lc.T, 4242)
    differs = np.unique(np.nonzero(x != plain)[0] // lc.BLOCK)
    assert set(differs) == set(lc.SPECIAL_BLOCKS) and len(lc.SPECIAL_BLOCKS) == 4
    b0, b2 = lc.SPECIAL_BLOCKS[0] * lc.BLOCK, lc.SPECIAL_BLOCKS[2] * lc.BLOCK
    assert (x[b0: b0 + lc.SPECIAL] == 0).all() and (x[b2: b2 + lc.SPECIAL] == 0xFF).all()
    for b in (lc.SPECIAL_BLOCKS[1], lc.SPECIAL_BLOCKS[3]):  # runs: far fewer changes of byte than bytes
        part = x[b * lc.BLOCK: b * lc.BLOCK + lc.SPECIAL]
        assert np.count_nonzero(np.diff(part)) < 64
    assert np.array_equal(lc.tail_of(x), x[: lc.TAIL])
    f = lc.tile("filter")
    assert len(f) == lc.T and not np.array_equal(f, x)
    sb = 8 * lc.BLOCK
    for s, w in ((8, 8), (9, 2), (10, 4)):  # minus_k: element k is -k
        e = f[s * sb: (s + 1) * sb].view(f"<u{w}")
        assert e[0] == 0 and e[1] == (1 << (8 * w)) - 1 and e[2] == (1 << (8 * w)) - 2
    assert len(np.unique(f[: 8 * sb])) == 256


@pytest.mark.parametrize("coder", lc.CODERS)
def test_the_payload_passes_4gib_too(oracle, coder):
    """The condition of large_cases: oracle sizes of the tile * 513 + the tail's stream > 2^32, for every coder."""
    p0, o0, pt, ot = lc.oracle_blocks(oracle, coder)
    assert len(o0) == lc.BLOCKS_PER_TILE + 1 and len(ot) == 2 and int(o0[-1]) == len(p0) and int(ot[-1]) == len(pt)
    total = lc.payload_bytes(oracle, coder)
    assert total == 513 * int(o0[-1]) + int(ot[-1])
    assert total > 1 << 32, (coder, total)
    # and the streams of period 512 lie wholly past 2^32, those of period 256 past 2^31
    assert 512 * len(p0) > 1 << 32 and 256 * len(p0) > 1 << 31
    # the special blocks' streams have sizes of their own: the table is not one number repeated
    assert len(set(np.diff(o0.astype(np.int64)).tolist())) >= 4


def test_the_item_pattern(oracle):
    p = lc.item_pattern()
    assert int(p.sum()) == lc.T and set(lc.ITEM_SPECIAL) <= set(p.tolist()) and int(p.max()) == 200_000
    t = lc.cut_to(p, lc.TAIL)
    assert int(t.sum()) == lc.TAIL and t.tolist()[:5] == [0, 1, 16, 17, 4097] and len(t) == 6
    full = lc.full_lengths(p, t)
    assert int(full.sum()) == lc.N and len(full) == lc.K * len(p) + len(t)
    items = lc.items_of(lc.tile("coder"), p)
    assert [len(x) for x in items] == p.tolist() and np.array_equal(np.concatenate(items), lc.tile("coder"))
    # the item streams of N bytes pass 2^32 as well (adaptive coder: the smallest streams of incompressible bytes)
    import gpu_support
    sizes = [0 if s is None else len(s) for s in gpu_support.oracle_streams(oracle, items, 0)]
    assert lc.K * sum(sizes) > 1 << 32


def test_typed_item_pattern_is_periodic():
    lengths, widths, preds = lc.typed_pattern()
    live = lengths > 0
    assert int(lengths.sum()) == lc.T and int((~live).sum()) == 210
    pairs = set(zip(widths[live].tolist(), preds[live].tolist()))
    assert pairs == {(w, p) for w in (2, 4, 8) for p in (0, 1, 2)}            # all three widths with all three predictors
    assert all(int(n) == int(w) * lc.BLOCK for n, w in zip(lengths[live], widths[live]))  # every item one superblock
    t, tw, tp = lc.cut_typed((lengths, widths, preds), lc.TAIL)
    assert t.tolist() == [lc.TAIL] and (int(tw[0]), int(tp[0])) == (8, 2) and lc.TAIL % 8 == 1
    # the expectation composed from predict_cases is the library's numpy mirror, item by item
    from cpprcoder_amd import typed_items
    case = {"lengths": lengths[:12], "widths": widths[:12], "preds": preds[:12]}
    x = lc.tile("filter")[: int(lengths[:12].sum())]
    offs = np.concatenate([[0], np.cumsum(lengths[:12])]).astype(np.uint64)
    assert np.array_equal(typed_items_cases.split_expected(case, x), typed_items.split_numpy(x, offs, widths[:12], preds[:12]))


# ---- the checkers must notice ------------------------------------------------------------------------------------------------
SMALL_BLOCK, SMALL_PERIODS = 16, 5


def small_instance(oracle, coder=0):
    """Tile of 4 blocks of 16 bytes, K = 5, a tail of 7 bytes; blocks 0 and 2 of the tile are chosen so that their streams are
    equally long and differ -> (tile, tail, payload0, offsets0, payload_tail, offsets_tail)."""
    for seed in range(200):
        x = workloads.uniform(4 * SMALL_BLOCK, seed)
        slots, sizes = oracle.encode_blocks(x, SMALL_BLOCK, coder=coder)
        if sizes[0] == sizes[2] and not np.array_equal(slots[0], slots[2]):
            break
    else:
        raise AssertionError("no seed gives two streams of equal length")
    p0, o0 = oracle.compact(slots, sizes)
    slots, sizes = oracle.encode_blocks(x[:7], SMALL_BLOCK, coder=coder)
    pt, ot = oracle.compact(slots, sizes)
    return x, x[:7], p0, o0, pt, ot


def build_small(oracle, offset=0):
    x, tail, p0, o0, pt, ot = small_instance(oracle)
    whole, view, table = lc.tiled_streams(p0, o0, pt, ot, periods=SMALL_PERIODS, offset=offset, device="cpu")
    return x, tail, p0, o0, view, table


@pytest.mark.parametrize("offset", [0, 3])
def test_the_builder_makes_what_the_oracle_makes_of_the_whole(oracle, offset):
    """tiled_streams against the oracle on the full (small) buffer: the payload, the table, and nothing written around them."""
    x, tail, p0, o0, pt, ot = small_instance(oracle)
    whole, view, table = lc.tiled_streams(p0, o0, pt, ot, periods=SMALL_PERIODS, offset=offset, device="cpu", guard=8)
    full = np.concatenate([np.tile(x, SMALL_PERIODS), tail])
    slots, sizes = oracle.encode_blocks(full, SMALL_BLOCK)
    want, want_offs = oracle.compact(slots, sizes)
    assert np.array_equal(view.numpy(), want) and np.array_equal(table.numpy(), want_offs.astype(np.int64))
    assert view.data_ptr() - whole.data_ptr() == 8 + offset and whole.numel() == 16 + offset + len(want)
    assert lc.all_bytes(whole[: 8 + offset], 0xA5) and lc.all_bytes(whole[8 + offset + len(want):], 0xA5)
    # and the checkers pass what is periodic
    P = lc.periodic_table(table, 4, SMALL_PERIODS)
    assert P == len(p0)
    lc.periodic_equal(view, P, SMALL_PERIODS)
    lc.periodic_equal(view.numpy(), P, SMALL_PERIODS)  # (the host-buffer test hands it numpy arrays)


@pytest.mark.parametrize("period", [1, 3, 4])
def test_a_one_byte_difference_is_named(oracle, period):
    _, _, p0, _, view, table = build_small(oracle)
    P = len(p0)
    view[period * P + P - 1] ^= 1  # the period's last byte
    with pytest.raises(AssertionError, match=rf"period {period} differs from period 0, first at byte {P - 1} "):
        lc.periodic_equal(view, P, SMALL_PERIODS)
    lc.periodic_table(table, 4, SMALL_PERIODS)  # (the table is untouched)
    # a step smaller than the periods: the loop's later turns see it as well
    with pytest.raises(AssertionError, match=rf"period {period} differs"):
        lc.periodic_equal(view, P, SMALL_PERIODS, step=1)


@pytest.mark.parametrize("period", [1, 4])
def test_a_table_row_off_by_one_is_named(oracle, period):
    _, _, p0, o0, view, table = build_small(oracle)
    table[period * 4 + 2] += 1
    want = int(o0[2] - o0[1]) if period else 0
    with pytest.raises(AssertionError, match=rf"period {period} differs from period 0 at entry 1: {want + 1} bytes, not {want}"):
        lc.periodic_table(table, 4, SMALL_PERIODS)
    # the period's FIRST entry off by one shows in the period in front (its last stream grows)
    _, _, _, _, _, table = build_small(oracle)
    table[period * 4] -= 1
    with pytest.raises(AssertionError, match=rf"period {period - 1} differs from period 0 at entry 3" if period > 1 else "period 1 differs"):
        lc.periodic_table(table, 4, SMALL_PERIODS)
    # a table that does not begin at 0, and one that is too short
    _, _, _, _, _, table = build_small(oracle)
    with pytest.raises(AssertionError, match="begins at 1"):
        lc.periodic_table(table + 1, 4, SMALL_PERIODS)
    with pytest.raises(AssertionError, match="entries"):
        lc.periodic_table(table[:20], 4, SMALL_PERIODS)


def test_a_swapped_pair_of_equal_length_streams_is_named(oracle):
    """Streams 0 and 2 of period 4 change places: the table cannot see it (they are equally long), the payload compare does."""
    _, _, p0, o0, view, table = build_small(oracle)
    P, period = len(p0), 4
    a, b, size = period * P + int(o0[0]), period * P + int(o0[2]), int(o0[1] - o0[0])
    assert size == int(o0[3] - o0[2])
    first, third = view[a: a + size].clone(), view[b: b + size].clone()
    assert not torch.equal(first, third)
    view[a: a + size], view[b: b + size] = third, first
    lc.periodic_table(table, 4, SMALL_PERIODS)
    with pytest.raises(AssertionError, match="period 4 differs from period 0"):
        lc.periodic_equal(view, P, SMALL_PERIODS)


def test_guards_and_all_bytes():
    whole = torch.full((100,), 0xA5, dtype=torch.uint8)
    view = whole[13: 13 + 50]
    assert lc.guards_intact(whole, view, written=0)
    view[:20] = 7
    assert lc.guards_intact(whole, view, written=20) and lc.guards_intact(whole, view) and not lc.guards_intact(whole, view, written=19)
    whole[12] = 0
    assert not lc.guards_intact(whole, view)
    whole[12], whole[63] = 0xA5, 1
    assert not lc.guards_intact(whole, view) and not lc.all_bytes(whole, 0xA5, step=7) and lc.all_bytes(whole[64:], 0xA5, step=7)
