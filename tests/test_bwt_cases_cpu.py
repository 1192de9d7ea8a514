"""What tests/test_gpu_bwt.py takes for granted about the blocks tests/bwt_cases.py builds for the forward kernel's switch
points (csrc/rcx_bwt.hpp, rcx_bwt_fwd_k), checked without a GPU: the ladders stand on every value around each list
length and around RUNNY, the run-keyed blocks are run-keyed and wrap where they should, and none is periodic (a
periodic block's row comes from the tie replay, not from the rounds).

bwt_cases.open_counts is a model of the kernel's `open`, derived from the code (rcx_bwt_rerank's `left`,
rcx_bwt_place's return value), not measured: the kernel cannot report the count.  The model itself is held here to a
definition-by-sorting on small inputs and to the closed form for planted repeats."""
import numpy as np
import pytest

import bwt_cases
from bwt_cases import BLOCK, LADDER_DEPTH, LIST_LENGTHS, ROTATIONS, RUNNY, changes, open_counts, primitive_period


def open_by_sorting(block, d):
    """The definition, the slow way: rotations cut to d bytes, counted as byte strings."""
    twice = np.concatenate([block, block]).tobytes()
    seen = {}
    for i in range(len(block)):
        seen[twice[i: i + d]] = seen.get(twice[i: i + d], 0) + 1
    return sum(v for v in seen.values() if v > 1)


def test_the_model_is_the_definition_on_small_blocks():
    for i, (n, alphabet) in enumerate(((64, 2), (256, 3), (1024, 4), (4096, 7), (4096, 256))):
        block = (bwt_cases.mix(n, 700 + i).astype(np.uint32) % alphabet).astype(np.uint8)
        got = open_counts(block)
        assert list(got) == [2 << k for k in range(len(got))]
        for d, v in got.items():
            assert v == open_by_sorting(block, d), (n, alphabet, d)
        last = max(got)
        assert got[last] == 0 or last == n   # it stops at the first depth where every rotation is alone
    assert open_counts(np.zeros(64, np.uint8)) == {2 << k: 64 for k in range(6)}          # period 1: never alone
    assert open_counts(np.arange(256, dtype=np.uint8)) == {2: 0}


def test_a_planted_repeat_opens_what_the_closed_form_says():
    """k copies of L bytes leave k (L - d + 1) rotations open at depth d >= 8 of a mix() block (below that, chance adds
    some); one byte more or fewer in the stretch moves the count by k, so the model sees an off-by-one."""
    for twice, thrice in ((519, 0), (520, 0), (9, 348), (9, 349), (5639, 0)):
        got = open_counts(bwt_cases.planted(40, twice, thrice))
        for d in (8, 16, 32, 64, 128, 256):
            want = 2 * max(twice - d + 1, 0) + 3 * max(thrice - d + 1, 0)
            assert got.get(d, 0) == want, (twice, thrice, d)
    assert open_counts(bwt_cases.planted(40, 5639))[8] == 11264 and open_counts(bwt_cases.planted(40, 1543))[8] == 3072
    assert open_counts(bwt_cases.planted(40, 519))[8] == 1024 and open_counts(bwt_cases.planted(40, 9, 1030))[8] == 3073
    assert open_counts(bwt_cases.planted(40, 8, 348))[8] == 1025


@pytest.mark.parametrize("limit", LIST_LENGTHS)
def test_a_ladder_stands_on_every_value_around_its_list_length(limit):
    ladder = bwt_cases.open_ladder(limit)
    assert len(ladder) == 7
    reached = set()
    for block in ladder:
        assert len(block) == BLOCK and block.dtype == np.uint8
        assert changes(block) >= RUNNY           # two-byte start: the model holds
        assert primitive_period(block) == BLOCK
        counts = open_counts(block)
        assert counts[max(counts)] == 0          # every rotation ends alone: the rounds do all the work
        reached |= {v for h, v in counts.items() if h >= 4}
    assert reached >= set(range(limit - 3, limit + 4))
    assert [open_counts(b)[LADDER_DEPTH] for b in ladder] == list(range(limit - 3, limit + 4))


def test_the_ladders_cross_every_form_of_a_round():
    """Between them the ladder blocks begin rounds with full passes and with each of the three list lengths, and each
    list length is met exactly full, one short and one over."""
    opens = [v for limit in LIST_LENGTHS for b in bwt_cases.open_ladder(limit) for h, v in open_counts(b).items() if v]
    assert any(v > 11264 for v in opens) and any(3072 < v < 11264 for v in opens)
    assert any(1024 < v < 3072 for v in opens) and any(v < 1024 for v in opens)
    for limit in LIST_LENGTHS:
        assert {limit - 1, limit, limit + 1} <= set(opens)


def test_the_runny_ladder_stands_on_every_value_around_the_threshold():
    ladder = bwt_cases.runny_ladder()
    assert [changes(b) for b in ladder] == list(range(RUNNY - 4, RUNNY + 5)) and RUNNY == 4096
    for i, block in enumerate(ladder):
        assert len(block) == BLOCK and block.dtype == np.uint8 and primitive_period(block) == BLOCK
        assert (block[0] == block[-1]) == bool(i % 2)    # every other one: a run round the block's end
    # changes() counts the wrap: a block whose last byte differs from its first has one more than its inner places
    b = ladder[0]
    assert changes(b) == int(np.count_nonzero(b[1:] != b[:-1])) + 1
    assert changes(np.zeros(BLOCK, np.uint8)) == 0 and changes(bwt_cases.cases()["ab..ab then aa"]) == BLOCK - 2


def test_the_run_key_cases_are_run_keyed_and_wrap():
    cases = bwt_cases.run_key_cases()
    assert len(cases) == 11 * (1 + len(ROTATIONS))
    for name, block in cases.items():
        assert len(block) == BLOCK and block.dtype == np.uint8, name
        assert changes(block) < RUNNY, name
        assert primitive_period(block) == BLOCK, name
        if "turned by" in name:
            assert block[0] == block[-1], name       # one run over the block's end
            base = cases[name.split(", turned by")[0]]
            assert np.array_equal(np.roll(block, -int(name.rsplit(" ", 1)[1])), base), name
    middle = cases["ones, a two in the middle"]
    assert int(np.argmax(middle)) == BLOCK // 2 and int(middle.sum()) == BLOCK + 1   # one run of 32767 that wraps


def test_aligned_and_tied_runs_are_what_their_names_say():
    block = bwt_cases.aligned_runs()
    ends = np.nonzero(block[1:] != block[:-1])[0] + 1
    starts = np.concatenate([[0], ends])
    lengths = np.diff(np.concatenate([starts, [BLOCK]]))
    have = {(int(n), int(s) % 32) for s, n in zip(starts, lengths)}
    assert have >= {(n, s) for n in (31, 32, 33, 63, 64, 65) for s in (0, 1, 31)}
    tied = bwt_cases.tied_runs()
    assert np.array_equal(tied[:28000], np.resize(np.repeat(np.array([97, 98], np.uint8), 20), 28000))
    assert 97 not in tied[28000:] and 98 not in tied[28000:]
    assert int(np.count_nonzero(tied[1:] == tied[:-1])) == BLOCK - changes(tied)   # (first and last byte differ)
