"""What tests/test_gpu_rans_shapes.py takes for granted about the inputs tests/rans_cases.py builds for the rANS kernels'
switch points (csrc/rcx_rans.hpp), checked without a GPU and with the oracle alone: the model of normalize() gives the
oracle's table for every block built, the victim blocks put the steal loop's victim into every lane's range, onto a tie
and through a change of victim, the dense runs press the encoders' output rings as hard as the formats can, and the
length sets give the rounds, groups, classes and residues their comments claim.

rans_cases.normalize_model and rans_cases.emitted are models read from the code (cppans.h as oracle/rans_oracle.c
restates it), used for aiming; neither is measured on the device, and neither is an expected value in a GPU test."""
import numpy as np
import pytest

import rans_cases
from rans_cases import (BITS, DENSE_RARE_HEADS, RANS1_WORKGROUP, WAVE_MIXED, WAVE_SAME_CLASS, WAVE_SAME_CLASS_PLUS_3, emitted,
                        item_class_upper, normalize_model, window_sums)

HEADER = 1032  # u32 n + 257 scaled cumulative counts (cppans.h:521, :598)


def counts_of(block):
    return np.bincount(block, minlength=256)


def header_of(oracle, block, simd):
    s = oracle.rans_encode(block, simd=simd)
    assert int(np.frombuffer(s[:4], "<u4")[0]) == len(block)
    return np.frombuffer(s[4:HEADER], "<u4")


@pytest.fixture(scope="module")
def blocks():
    return rans_cases.block_cases()


@pytest.fixture(scope="module")
def dense(oracle):
    """(head, simd) -> (per-symbol output of the model, the oracle's stream length)."""
    return {(h, simd): (emitted(rans_cases.dense_rare(h), simd), len(oracle.rans_encode(rans_cases.dense_rare(h), simd=simd)))
            for h in DENSE_RARE_HEADS for simd in (False, True)}


# ---- the model of normalize() ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("simd", [False, True], ids=["14 bits", "12 bits"])
def test_the_model_gives_the_oracles_table_for_every_block_built(oracle, blocks, simd):
    assert len(blocks) == 18 + 1 + 6 + 8 + 2
    for name, block in blocks.items():
        assert block.dtype == np.uint8 and len(block) <= rans_cases.PADDED_BLOCK, name
        cum, events = normalize_model(counts_of(block), BITS[simd])
        assert np.array_equal(cum, header_of(oracle, block, simd)), name
        assert cum[0] == 0 and cum[256] == 1 << BITS[simd], name
        ranges = np.diff(cum.astype(np.int64))
        assert np.array_equal(ranges > 0, counts_of(block) > 0), name           # every symbol that occurs has a slot
        assert all(0 <= v < 256 and r > 1 and v != i for i, v, r in events), name   # a victim there always is; never the loser itself


def test_the_model_on_small_trials(oracle):
    """Random counts over a few symbols, some of them once in a long block: the table is the oracle's at both widths."""
    rs = np.random.RandomState(5)
    stolen = 0
    for trial in range(40):
        counts = np.zeros(256, np.int64)
        used = rs.choice(256, int(rs.randint(2, 200)), replace=False)
        counts[used] = rs.randint(1, 4, len(used))
        counts[used[0]] = int(rs.randint(5000, 40000))
        if trial % 2:
            counts[used[1]] = int(rs.randint(2, 60))   # a small victim somewhere
        block = rans_cases.from_counts(counts, trial)
        for simd in (False, True):
            cum, events = normalize_model(counts, BITS[simd])
            assert np.array_equal(cum, header_of(oracle, block, simd)), (trial, simd)
            stolen += len(events)
    assert stolen > 1000


def test_the_victim_blocks_cover_every_lane_a_tie_and_a_change_of_victim():
    cases = rans_cases.victim_cases()
    assert list(cases) == [f"lane {k}" for k in range(8)] + [f"tie {k}" for k in range(8)] + ["dominant 0", "dominant 255"]
    for simd in (False, True):
        bits = BITS[simd]
        lanes_hit, directions, small_directions, ties, changes = set(), set(), set(), 0, 0
        for lane in range(8):
            block = cases[f"lane {lane}"]
            counts, first, second = rans_cases.victim_counts(lane)
            assert np.array_equal(counts_of(block), counts) and len(block) == rans_cases.LOSER_BLOCK > 1 << bits
            assert {first, second} == {32 * lane + 31, (32 * lane + 32) % 256} and first // 32 != second // 32   # across a lane border
            losers = np.nonzero(counts == 1)[0]
            assert (first < losers.min() and losers.max() < second) if lane == 7 else (losers.min() < first and losers.max() > second)   # on both sides of each victim
            cum, events = normalize_model(counts, bits)
            ranges = np.diff(normalize_scaled(counts, bits))
            small = int(ranges[first])
            assert ranges[first] == ranges[second] == (counts[first] << bits) // len(block) and 2 <= small <= 12   # the tie, before any steal
            assert small == min(r for r in ranges if r > 1)
            assert events[0][1:] == (first, small)                                     # ... goes to the lower index
            ties += 1
            assert all(counts[i] == 1 for i, _, _ in events)                           # only the symbols that occur once lose
            victims = [v for _, v, _ in events]
            dominant = int(np.argmax(counts))
            # worn to 1, the first victim is left alone: the second follows, then the dominant symbol
            assert victims == [first] * (small - 1) + [second] * (small - 1) + [dominant] * (len(events) - 2 * (small - 1))
            assert len(events) > 2 * (small - 1)
            assert [r for _, v, r in events if v == first] == list(range(small, 1, -1))
            changes += sum(1 for a, b in zip(victims, victims[1:]) if a != b)
            assert cum[first + 1] - cum[first] == 1 and cum[second + 1] - cum[second] == 1
            lanes_hit |= {v // 32 for v in victims}
            directions |= {v < i for i, v, _ in events}
            small_directions |= {v < i for i, v, _ in events if v != dominant}
        assert lanes_hit == set(range(8)) and directions == small_directions == {True, False} and ties == 8 and changes == 16
        for lane in range(8):
            # two losers at the most: the tie's winner alone is worn, and the table shows which it was
            counts, first, second = rans_cases.tie_counts(lane)
            assert np.array_equal(counts_of(cases[f"tie {lane}"]), counts) and int(counts.sum()) == rans_cases.LOSER_BLOCK
            assert {first, second} == {32 * lane + 31, (32 * lane + 32) % 256} and np.count_nonzero(counts == 1) == 2
            before = np.diff(normalize_scaled(counts, bits))
            cum, events = normalize_model(counts, bits)
            after = np.diff(cum.astype(np.int64))
            assert before[first] == before[second] == min(r for r in before if r > 1)
            assert 1 <= len(events) <= 2 and all(v == first for _, v, _ in events)
            assert after[first] == before[first] - len(events) < after[second] == before[second]
        for name, dominant, toward_lower in (("dominant 0", 0, True), ("dominant 255", 255, False)):
            counts = counts_of(cases[name])
            _, events = normalize_model(counts, bits)
            assert int(np.argmax(counts)) == dominant and int(counts.sum()) == rans_cases.LOSER_BLOCK
            assert len(events) >= 40 and all((v, v < i) == (dominant, toward_lower) for i, v, _ in events), name


def normalize_scaled(counts, bits):
    """The scaled cumulative counts before any steal (cppans.h:142)."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    return (cum << bits) // cum[-1]


def test_singletons_steal_196_and_240_slots_from_symbol_128(oracle):
    block = rans_cases.singletons()
    counts = counts_of(block)
    assert len(block) == 70255 and counts[128] == 70000 and np.count_nonzero(counts == 1) == 255
    for simd, steals in ((False, 196), (True, 240)):
        cum, events = normalize_model(counts, BITS[simd])
        assert np.array_equal(cum, header_of(oracle, block, simd))
        assert len(events) == steals and {v for _, v, _ in events} == {128}
        assert {v < i for i, v, _ in events} == {True, False}
        assert [r for _, _, r in events] == list(range(events[0][2], events[0][2] - steals, -1))   # every step sees the one before


# ---- what leaves the encoders, and how fast ------------------------------------------------------------------------------------
def test_emitted_adds_up_to_the_oracles_stream(oracle, dense):
    for (head, simd), (per_symbol, stream_len) in dense.items():
        assert len(per_symbol) == head + 70255
        if simd:
            assert 2 * int(per_symbol.sum()) == stream_len - (HEADER + 32) and per_symbol.max() == 1, head
        else:
            assert int(per_symbol.sum()) == stream_len - (HEADER + 4) and per_symbol.max() == 2, head
    for block in (rans_cases.one_symbol(9), rans_cases.one_symbol(4096), rans_cases.all_256(3), rans_cases.victim_cases()["lane 3"]):
        for simd in (False, True):
            total = int(emitted(block, simd).sum()) * (2 if simd else 1)
            assert total == len(oracle.rans_encode(block, simd=simd)) - HEADER - (32 if simd else 4)
    assert int(emitted(rans_cases.one_symbol(4096), True).sum()) == 4096       # frequency 4096: x_max wraps to 0, a word for every symbol
    assert int(emitted(rans_cases.one_symbol(4096), False).sum()) == 0          # frequency 16384: nothing ever leaves


@pytest.mark.parametrize("head", DENSE_RARE_HEADS)
def test_dense_runs_press_the_output_rings(dense, head):
    """Conditions, not targets: a chunk of 16 symbols with at least 26 bytes (the one-state encoders' 64-byte ring takes 32
    at the most), eight rounds with at least 90 bytes and a round of 8 words (the eight-state encoder's 256-byte ring
    takes 128).  The reference gives 28, 96 and 8 at every head; 15 or 16 chunks and 3 or 4 groups reach the levels."""
    bytes_by_chunk = window_sums(dense[head, False][0], 16)
    words = dense[head, True][0]
    bytes_by_group, words_by_round = 2 * window_sums(words, 64), window_sums(words, 8)
    assert bytes_by_chunk.max() >= 26 and bytes_by_group.max() >= 90 and words_by_round.max() == 8
    assert (bytes_by_chunk.max(), bytes_by_group.max()) == (28, 96)
    assert int(np.count_nonzero(bytes_by_chunk >= 26)) in (15, 16) and int(np.count_nonzero(bytes_by_group >= 90)) in (3, 4)
    assert bytes_by_chunk.max() <= 32 and bytes_by_group.max() <= 128     # what the rings are sized for
    run_at = head + 40000
    assert {(h + 40000) % 8 for h in DENSE_RARE_HEADS} == {0, 1, 7} and {(h + 40000) % 16 for h in DENSE_RARE_HEADS} == {0, 1, 7, 8, 15}
    block = rans_cases.dense_rare(head)
    assert len(set(block[run_at: run_at + 255].tolist())) == 255 and not block[:run_at].any() and not block[run_at + 255:].any()


# ---- the length sets ---------------------------------------------------------------------------------------------------------
def starts(lengths, offset=0):
    return offset + np.concatenate([[0], np.cumsum(lengths)[:-1]])


def test_item_class_upper_is_the_power_of_two_at_or_above():
    assert [item_class_upper(n) for n in (1, 15, 16, 17, 32, 33, 512, 513, 1024, 1025)] == [16, 16, 16, 32, 32, 64, 512, 1024, 1024, 2048]


def test_same_class_is_one_aligned_wave():
    lengths = WAVE_SAME_CLASS
    assert len(lengths) == 8 and lengths == sorted(lengths, reverse=True) and rans_cases.work_order(lengths) == list(range(8))
    assert {item_class_upper(n) for n in lengths} == {1024}                       # one launch, one wave of eight octets
    assert all(n % 8 == 0 for n in lengths[:-1]) and lengths[-1] % 8 == 3
    for offset in (0, 8):
        assert all(s % 8 == 0 for s in starts(lengths, offset))                   # by_eights, out8
    after_last = [(n + 7) // 8 - 1 for n in lengths]                              # rounds behind each block's last, maybe short, one
    assert min(after_last) == 64 and max(after_last) + 1 == 128                   # `common`, below the longest block's 128 rounds
    assert sorted({r & 7 for r in after_last}) == [0, 4, 7]                       # rounds above a multiple of eight: some, and none
    groups = [n >> 3 for n in lengths]
    assert min(g & ~7 for g in groups) == 64 and max(groups) == 128               # fast_groups, max_groups
    assert any(g & 7 for g in groups) and sorted({n & 7 for n in lengths}) == [0, 3]


def test_same_class_plus_3_is_aligned_nowhere():
    lengths = WAVE_SAME_CLASS_PLUS_3
    assert lengths == [n + 3 for n in WAVE_SAME_CLASS]
    assert [item_class_upper(n) for n in lengths] == [2048] + [1024] * 7          # 1027 is a class of its own
    for offset in (0, 8, 1):
        off_border = [int(s) % 8 != 0 for s in starts(lengths, offset)]
        assert sum(off_border) >= 7                                               # by_eights fails, and fast_groups is 0
        assert sum(off_border[1:]) >= 6                                           # (in the wave of seven as well)


def test_mixed_puts_4096_next_to_1():
    lengths = WAVE_MIXED
    assert lengths == sorted(lengths, reverse=True) and len(lengths) == 13 and (max(lengths), min(lengths)) == (4096, 1)
    assert sorted({n & 7 for n in lengths}) == [0, 1, 5, 7]                       # the tails behind the last whole group
    groups = [n >> 3 for n in lengths]
    assert any(g and g & 7 == 0 for g in groups) and any(g & 7 for g in groups) and groups.count(0) == 2
    per_class = {}
    for n in lengths:
        per_class[item_class_upper(n)] = per_class.get(item_class_upper(n), 0) + 1
    assert per_class == {4096: 1, 2048: 1, 1024: 1, 256: 1, 128: 1, 64: 2, 32: 1, 16: 5}   # every encoder wave has idle octets
    # the decoders' waves: eight blocks each for the eight-state one; 16 or 4 for the one-state one where the tests force it
    assert [lengths[w: w + 8] for w in (0, 8)] == [[4096, 1029, 520, 129, 72, 64, 63, 17], [16, 9, 8, 7, 1]]
    assert rans_cases.quad_waves(lengths, 16) == [lengths]
    assert rans_cases.quad_waves(lengths, 4) == [[4096, 1029, 520, 129], [72, 64, 63, 17], [16, 9, 8, 7], [1]]
    assert rans_cases.quad_waves(lengths, 1) == [[n] for n in lengths]           # (the default shape of so small a call: nothing side by side)
    assert rans_cases.quad_waves(lengths[::-1], 16) == [lengths]                 # the work order, whatever the caller's


def test_the_rans1_workgroup_ends_at_every_place_of_a_chunk():
    lengths = RANS1_WORKGROUP
    assert len(lengths) == 64 and {item_class_upper(n) for n in lengths} == {512} and all(256 < n <= 512 for n in lengths)
    assert sorted(n % 16 for n in lengths) == sorted(list(range(16)) * 4)
    chunks = [(n + 15) // 16 for n in lengths]
    assert max(chunks) == 32 and min(chunks) == 21 and lengths[0] == max(lengths)  # nchunks follows the longest, in lane 0
    assert rans_cases.work_order(lengths) == list(range(64))
    for quads, waves in ((16, 4), (4, 16)):                                        # the one-state decoder's waves, forced
        seated = rans_cases.quad_waves(lengths, quads)
        assert len(seated) == waves and all(len(set(w)) == quads for w in seated)  # no two lengths of a wave are equal
        assert all(max(w) - min(w) == 3 * (quads - 1) for w in seated)
    assert all(len({(n + 15) // 16 for n in w}) >= 3 for w in rans_cases.quad_waves(lengths, 16))   # several 16-symbol pieces apart
    assert [len(set(w)) for w in rans_cases.quad_waves(WAVE_SAME_CLASS, 16)] == [8]


def test_rare_items_are_runs_of_different_bytes_among_zeros():
    for n in (1, 7, 8, 17, 129, 520, 4096):
        item = rans_cases.rare_item(n, n)
        m = min(255, n // 2)
        other = item[item != 0]
        assert len(item) == n and len(other) == m == len(set(other.tolist()))
        assert m == 0 or np.array_equal(item[(n - m) // 2: (n - m) // 2 + m], other)


@pytest.mark.parametrize("filler", ["seeded", "dominant"])
def test_the_padded_call_keeps_every_block_at_its_place(blocks, filler):
    block = rans_cases.PADDED_BLOCK
    data = rans_cases.padded_call(blocks, filler)
    assert len(data) == len(blocks) * block and np.array_equal(data, rans_cases.padded_call(blocks, filler))
    steals = {bits: [] for bits in (14, 12)}
    names = list(blocks)
    for b, k in enumerate(rans_cases.padded_order(len(names))):
        case = blocks[names[k]]
        assert np.array_equal(data[b * block: b * block + len(case)], case)
        for bits in steals:
            steals[bits].append(len(normalize_model(counts_of(data[b * block: (b + 1) * block]), bits)[1]))
    for bits, per_block in steals.items():
        if filler == "seeded":
            assert not any(per_block)               # (the filler gives every symbol a range: the models differ, nothing is stolen)
        else:
            waves = [per_block[w: w + 8] for w in range(0, len(per_block), 8)]   # eight blocks to a wave, each its own steal loop
            assert max(per_block) >= 200 and min(per_block) == 0, (bits, per_block)
            assert all(len(set(w)) >= 4 and max(w) >= 37 and min(w) <= 2 for w in waves[:-1]), (bits, waves)
