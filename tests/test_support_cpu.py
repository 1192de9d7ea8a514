"""The shared test support (tests/gpu_support.py) held to its contract, on CPU tensors: every "writes nothing outside
its buffer" claim of the GPU tests rests on Guarded.check failing when it should, their launch shapes on knobs leaving the
environment as it found it, their parity claims on the two comparisons, and the threaded scenarios of
tests/test_gpu_threads.py on run_together (held here with sleeping jobs)."""
import os
import threading
import time

import numpy as np
import pytest

from gpu_support import (GUARD, SHAPE_EDGE_IDS, Guarded, assert_same_blocks, assert_same_items, chunk_blocks, decode_quads, encode_lanes,
                         jobs_intersect, knobs, library_call, run_alone, run_together, shape_edges, stuck_message)

SIZES, OFFSETS = (0, 1, 33), (0, 15)


def guarded(size, offset, invert=False):
    return Guarded(size, offset, np.arange(size, dtype=np.uint8), salt=2, invert=invert, device="cpu")


@pytest.mark.parametrize("invert", [False, True])
def test_an_untouched_buffer_passes(invert):
    for size in SIZES:
        for offset in OFFSETS:
            g = guarded(size, offset, invert)
            assert g.view.numel() == size and g.view.tolist() == list(range(size))
            assert g.tensor.numel() == GUARD + offset + size + GUARD
            g.check(0)
            g.check(size)
            g.view.fill_(0)  # the call wrote all it may
            g.check(size)


def changed(g, position, written):
    """check(written) after one byte at `position` (relative to the buffer) changed -> the AssertionError's text."""
    g.tensor[g.at + position] ^= 0x40
    with pytest.raises(AssertionError) as e:
        g.check(written, "dst")
    return str(e.value)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("size", SIZES)
def test_one_changed_byte_outside_what_may_be_written_fails(size, offset):
    for written in sorted({0, size // 2, size}):
        for position in (-1, -(GUARD + offset), written, size + GUARD - 1):
            msg = changed(guarded(size, offset), position, written)
            assert msg.startswith(f"dst: byte {position} changed") and f"the {written} bytes" in msg, msg
    if size:  # an input: none of its bytes may change
        for position in (0, size - 1):
            assert f"byte {position} changed" in changed(guarded(size, offset), position, 0)


def test_the_lowest_changed_byte_is_named():
    g = guarded(33, 15)
    g.tensor[g.at + 40] ^= 1
    assert "byte 20 changed" in changed(g, 20, 10)
    g.tensor[g.at - 3] ^= 1
    with pytest.raises(AssertionError, match="byte -3 changed"):
        g.check(10)


def test_the_pattern_is_nonzero_and_differs_by_salt_and_inversion():
    images = {}
    for salt in (1, 2):
        for invert in (False, True):
            t = Guarded(1000, 3, salt=salt, invert=invert, device="cpu").tensor.numpy()
            assert t.min() >= 1, (salt, invert)  # (251 + 1 at the most, so the complement is nonzero too)
            images[salt, invert] = t
    assert np.array_equal(images[1, True], ~images[1, False])
    keys = list(images)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert np.count_nonzero(images[a] != images[b]) > 900, (a, b)


class Boom(Exception):
    pass


@pytest.mark.parametrize("fail", [False, True])
def test_knobs_restore_the_environment(monkeypatch, fail):
    monkeypatch.setenv("RCX_T_SET", "before")
    monkeypatch.setenv("RCX_T_CLEARED", "kept")
    monkeypatch.delenv("RCX_T_UNSET", raising=False)
    monkeypatch.delenv("RCX_T_CLEARED_UNSET", raising=False)
    whole = dict(os.environ)
    try:
        with knobs({"RCX_T_SET": "inside", "RCX_T_UNSET": "1"}, clear=("RCX_T_CLEARED", "RCX_T_CLEARED_UNSET")):
            assert os.environ["RCX_T_SET"] == "inside" and os.environ["RCX_T_UNSET"] == "1"
            assert "RCX_T_CLEARED" not in os.environ and "RCX_T_CLEARED_UNSET" not in os.environ
            if fail:
                raise Boom
    except Boom:
        assert fail
    assert dict(os.environ) == whole
    # a variable both cleared and set is set inside, and back to what it was afterwards
    with knobs({"RCX_T_CLEARED": "2"}, clear=("RCX_T_CLEARED",)):
        assert os.environ["RCX_T_CLEARED"] == "2"
    assert dict(os.environ) == whole


def test_chunk_blocks_restates_host_chunk_blocks():
    """csrc/rcx_host.hpp host_chunk_blocks(), by hand: 2048 (encode) or 4096 (decode) blocks, at least 16 MiB worth, doubled
    until there are at most 2048 chunks, then equal chunks, rounded up to a multiple of 64."""
    for (block, decode, nblocks), want in {
        (4096, True, 100): 4096,            # one chunk: the floor of 16 MiB / 4096 itself
        (4096, False, 100): 4096,           # (the encoder's 2048 is below that floor)
        (65536, False, 100): 2048,          # the floor is 256 blocks: the defaults stand
        (65536, True, 100): 4096,
        (16, True, 1): 1 << 20,             # 16 MiB of 16-byte blocks
        (4096, True, 9092): 3072,           # 3 chunks of 4096 -> 3031 each -> the next multiple of 64
        (4096, False, 22785): 3840,         # 6 chunks -> 3798 each -> 3840
        (65536, False, 4273): 1472,         # 3 chunks of 2048 -> 1425 each -> 1472
        (65536, True, 16384): 4096,         # 4 equal chunks exactly
        (1 << 20, True, 1 << 23): 4096,     # 2048 chunks: the most there may be
        (1 << 20, True, (1 << 23) + 1): 8192,  # one block more: 8192 a chunk, 1025 chunks of 8185 -> 8192
    }.items():
        assert chunk_blocks(block, decode, nblocks) == want, (block, decode, nblocks)


@pytest.mark.parametrize("cus", [256, 304])
def test_shape_edges_sit_on_every_change_of_launch_shape(cus):
    """csrc/rcx_launch.hpp encode_lanes() / decode_quads(), by hand, and the counts tests/test_gpu_launch_shapes.py walks:
    one block more than each multiple changes the shape, so a list without m + 1 would miss the change."""
    edges = shape_edges(cus)
    assert len(edges) == len(SHAPE_EDGE_IDS) == 21 and len(set(SHAPE_EDGE_IDS)) == 21
    for k, quads in ((1, 1), (2, 2), (4, 4), (8, 8)):
        m = 4 * cus * k
        assert (decode_quads(m - 1, cus), decode_quads(m, cus), decode_quads(m + 1, cus)) == (quads, quads, 2 * quads), m
        assert {m - 1, m, m + 1} <= set(edges)
    for k in (1, 2, 4, 8, 16, 32):
        m = cus * k
        assert (encode_lanes(m, cus), encode_lanes(m + 1, cus)) == (k, 2 * k), m
        assert encode_lanes(m - 1, cus) == k or k == 1
        assert {m - 1, m, m + 1} <= set(edges)
    assert decode_quads(1, cus) == encode_lanes(1, cus) == 1
    assert decode_quads(1 << 20, cus) == 16 and encode_lanes(1 << 20, cus) == 64          # the caps
    assert {32767, 32768, 32769} <= set(edges)
    assert edges == sorted(edges) or cus * 32 > 32767    # (in ascending order where the device is no larger than 1023 CUs)


def test_shape_edges_of_256_compute_units():
    edges = shape_edges(256)
    assert {1025, 8193, 32768} <= set(edges) and edges[:4] == [255, 256, 257, 511] and min(shape_edges(1)) == 1
    assert [decode_quads(n, 256) for n in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert [encode_lanes(n, 256) for n in (256, 257, 8192, 8193, 32768)] == [1, 2, 32, 64, 64]
    # neither power-of-two rounding nor the cap is taken for granted: 3 workgroups' worth rounds up to 4
    assert encode_lanes(3 * 256, 256) == 4 and decode_quads(3 * 1024, 256) == 4 and decode_quads(5 * 1024, 256) == 8


def four_blocks():
    sizes = np.array([5, 7, 3, 6], np.uint32)
    slots = np.arange(4 * 16, dtype=np.uint8).reshape(4, 16) + 1
    streams = [slots[b, : int(sizes[b])] for b in range(4)]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return np.concatenate(streams), offsets, slots, sizes, streams


def test_the_comparisons_fail_when_they_should():
    payload, offsets, slots, sizes, streams = four_blocks()
    assert_same_blocks(payload, offsets, slots, sizes)
    assert_same_items(payload, offsets, streams)
    # an item of length 0 has no stream
    assert_same_items(payload, np.insert(offsets, 2, offsets[2]), streams[:2] + [None] + streams[2:])
    # a size mismatch: a byte moves from block 1 to block 2
    moved = offsets.copy()
    moved[2] -= 1
    with pytest.raises(AssertionError, match="sizes differ"):
        assert_same_blocks(payload, moved, slots, sizes)
    with pytest.raises(AssertionError, match="sizes"):
        assert_same_items(payload, moved, streams)
    with pytest.raises(AssertionError, match="sizes"):
        assert_same_items(payload, offsets, streams[:2] + [None] + streams[3:])
    # one byte of a middle block differs
    for at, b in ((int(offsets[2]), 2), (int(offsets[2]) - 1, 1)):
        bad = payload.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError, match=f"here: block {b} differs"):
            assert_same_blocks(bad, offsets, slots, sizes, "here")
        with pytest.raises(AssertionError, match=f"here: item {b} differs"):
            assert_same_items(bad, offsets, streams, "here")


# ---- tests/resumable_cases.py: what the GPU tests of the resumable coders take for granted about their inputs -------------
def test_a_constant_piece_ends_at_the_halving():
    import resumable_cases as rc
    from golden_cases import LONG_ADAPTIVE, NO_HALVING
    assert rc.H == NO_HALVING == (1 << 24) - 256 and NO_HALVING % 1_048_560 == 0 and rc.HALVING_PIECE == 1_048_560
    assert rc.LONG_UNIFORM in LONG_ADAPTIVE and rc.LONG_MIN_ZIPF in LONG_ADAPTIVE
    sizes = rc.around_halving(NO_HALVING + 5000)
    assert sizes == [NO_HALVING - 1, 1, 1, 4999] and sum(sizes) == NO_HALVING + 5000
    assert rc.constant(10, 4) == [4, 4, 2] and rc.split(b"abcdefghij", [4, 4, 2]) == [b"abcd", b"efgh", b"ij"]
    assert sum(rc.uneven(311_564)) == 311_564 and rc.uneven(311_564)[:5] == [100_000, 1, 1, 70_000, 8]


def test_the_carry_input_outgrows_the_facades_guess(oracle):
    import resumable_cases as rc
    data = rc.carry_input()
    assert len(data) == rc.CARRY_N
    (st, rq), sink, sizes = oracle.adaptive_encode_trace(data, rc.CARRY_PIECE)
    jumps = np.diff(sizes)
    assert (st, rq) == (0, 0) and int(jumps.max()) > 3 * 64 + 4096 == rc.FACADE_ROOM
    assert int(np.count_nonzero(jumps > rc.FACADE_ROOM)) == 1
    # the writer restated in resumable_cases agrees with the oracle about where the run ends, and how
    j = rc.carrying_symbol(data)
    assert j // rc.CARRY_PIECE == int(np.argmax(jumps))
    assert b"\x00" * (rc.CARRY_RUN - 1) in sink and b"\xff" * rc.CARRY_RUN not in sink


def test_the_altered_piece_does_not_carry(oracle):
    import resumable_cases as rc
    data = rc.carry_input()
    altered, j = rc.without_the_carry(data)
    assert len(altered) == len(data) and np.array_equal(altered[:j], data[:j]) and altered[j] != data[j]
    long_runs = [e for e in rc.writer_events(altered) if e[1] >= rc.CARRY_RUN]
    assert len(long_runs) == 1 and long_runs[0][0] == j and not long_runs[0][2]  # the run ends in symbol j, by a smaller byte
    assert b"\xff" * rc.CARRY_RUN in oracle.adaptive_encode(altered)[1]


def test_the_launch_loop_input_is_long_and_codes_small(oracle):
    import resumable_cases as rc
    v = rc.loop_input()
    assert len(v) == rc.LOOP_N == 2_621_440 == 5 * rc.CHUNK // 2 and int(v.max()) == 3
    assert len(oracle.adaptive_encode(v)[1]) < 1_000_000
    assert [-(-rc.LOOP_N // cap) for cap in rc.LOOP_CAPS + (rc.LOOP_ONE_CALL,)] == [3, 3, 3, 2, 1]
    kinds = [(k, len(b)) for k, b, _ in rc.interleaved_inputs()]
    assert [k for k, _ in kinds] == ["dec", "enc", "dec", "enc"] and all(20_000 <= n <= 70_000 for _, n in kinds)


# ---- run_together: what tests/test_gpu_threads.py takes for granted about its threads ---------------------------------------
class Sleeper:
    """A job that sleeps `naps[round]` seconds and notes when each round began and ended, and on which thread."""

    def __init__(self, naps, fail_in=None):
        self.naps, self.fail_in = naps, fail_in
        self.began, self.ended, self.threads = [], [], set()

    def setup(self):
        self.threads.add(threading.get_ident())

    def __call__(self, r):
        self.threads.add(threading.get_ident())
        self.began.append(time.perf_counter())
        if r == self.fail_in:
            raise Boom("went wrong")
        time.sleep(self.naps[r])
        self.ended.append(time.perf_counter())

    def close(self):
        self.threads.add(threading.get_ident())
        self.closed = True


def test_run_together_names_the_job_and_the_round_of_the_first_exception():
    jobs = [Sleeper([0.01] * 3), Sleeper([0.01] * 3), Sleeper([0.01] * 3, fail_in=1)]
    with pytest.raises(AssertionError, match=r"job 2, round 1: Boom: went wrong") as e:
        run_together(jobs, 3, limit=30)
    assert isinstance(e.value.__cause__, Boom)
    # nobody went on into round 2; every job, the failing one too, was closed, and on its own thread
    assert len(jobs[2].began) == 2 and all(len(j.began) <= 2 for j in jobs)
    assert all(j.closed and len(j.threads) == 1 for j in jobs)
    # an exception in the set-up step is named as such
    class BadSetup(Sleeper):
        def setup(self):
            raise Boom("no context")
    pair = [Sleeper([0.01]), BadSetup([0.01])]
    with pytest.raises(AssertionError, match=r"job 1, set-up: Boom: no context"):
        run_together(pair, 1, limit=30)
    assert pair[0].closed and not hasattr(pair[1], "closed")  # (a job whose set-up failed has nothing to close)
    with pytest.raises(AssertionError, match=r"alone: job 1: Boom: no context"):
        run_alone([Sleeper([0.0]), BadSetup([0.0])], 1)


def test_run_together_reports_a_job_that_is_not_back_in_time():
    class Stuck(Exception):
        pass

    def stuck(message):
        raise Stuck(message)

    # (wide margins, for a loaded machine: round 0 has 2 s, and the nap of round 1 outlasts the limit by far; the
    # sleeping thread is a daemon and is left behind)
    jobs = [Sleeper([0.01, 0.01]), Sleeper([0.01, 20.0])]
    with pytest.raises(Stuck, match=r"job 1 \(round 1\) not back after 2 s") as e:
        run_together(jobs, 2, limit=2, stuck=stuck)
    assert "job 0" not in str(e.value)  # (it was back from round 1, or waiting for nobody)
    assert stuck_message([(0, "round 3"), (2, "set-up")], 120).startswith("run_together: job 0 (round 3), job 2 (set-up) not back after 120 s")
    # by default the report ends the session: pytest.exit, not a failure that lets later tests start more GPU work
    import gpu_support
    import inspect
    assert inspect.signature(run_together).parameters["stuck"].default is gpu_support._end_the_session
    with pytest.raises(pytest.exit.Exception, match="hangs"):
        gpu_support._end_the_session(stuck_message([(1, "round 0")], 120))


def test_intersecting_and_disjoint_intervals_are_told_apart():
    def intervals_intersect(spans):  # one span per job, None for a job that did not run
        return jobs_intersect([s and [s] for s in spans])

    assert intervals_intersect([(0.0, 1.0), (0.5, 2.0)])
    assert intervals_intersect([(0.0, 5.0), (1.0, 2.0), (7.0, 8.0)])        # one inside another
    assert intervals_intersect([(3.0, 4.0), (0.0, 1.0), (3.5, 3.6)])        # in any order
    assert not intervals_intersect([(0.0, 1.0), (1.0, 2.0), (2.5, 3.0)])    # touching is not intersecting
    assert not intervals_intersect([(0.0, 1.0)]) and not intervals_intersect([]) and not intervals_intersect([(0.0, 1.0), None])
    assert intervals_intersect([(0.0, 10.0), (1.0, 2.0), (5.0, 6.0)])       # the long one reaches over both
    # and through run_together: two sleepers side by side overlap in every round; a job alone never does
    assert run_together([Sleeper([0.05] * 2), Sleeper([0.05] * 2)], 2, limit=30) == [True, True]
    assert run_together([Sleeper([0.01] * 2)], 2, limit=30) == [False, False]


class Caller(Sleeper):
    """A job that spends `naps[round]` seconds outside any call and then, if `calls`, 0.05 s in library_call()."""

    def __init__(self, naps, calls=True):
        super().__init__(naps)
        self.calls = calls

    def __call__(self, r):
        super().__call__(r)
        if self.calls:
            with library_call():
                time.sleep(0.05)


def test_only_the_time_inside_the_library_counts_as_overlap():
    assert jobs_intersect([[(0.0, 1.0)], [(0.5, 2.0)]])
    assert not jobs_intersect([[(0.0, 1.0), (0.5, 2.0)], None, []])                # two spans of ONE job
    assert not jobs_intersect([[(0.0, 1.0), (4.0, 5.0)], [(1.0, 2.0), (3.0, 4.0)]])  # touching is not intersecting
    assert jobs_intersect([[(0.0, 1.0), (4.0, 5.0)], [(2.0, 3.0), (4.5, 4.6)]])
    assert jobs_intersect([[(0.0, 10.0)], [(1.0, 2.0)], [(5.0, 6.0)]]) and jobs_intersect([[(1.0, 2.0), (3.0, 9.0)], [(0.0, 0.5), (8.0, 8.5)]])
    assert not jobs_intersect([]) and not jobs_intersect([[(0.0, 1.0)]])
    # the rounds intersect as wholes, but the calls inside do not: one job's call is over long before the other's begins
    assert run_together([Caller([0.0] * 2), Caller([1.0] * 2)], 2, limit=60, calls_only=True) == [False, False]
    assert run_together([Caller([0.0] * 2), Caller([0.0] * 2)], 2, limit=60, calls_only=True) == [True, True]
    # a job without any such span counts with its whole round, unless the caller asks for calls only
    assert run_together([Caller([0.0]), Caller([0.3], calls=False)], 1, limit=60) == [True]
    with pytest.raises(AssertionError, match=r"job 1, round 0: AssertionError: the job went through no library_call"):
        run_together([Caller([0.0]), Caller([0.0], calls=False)], 1, limit=60, calls_only=True)
    with library_call():  # outside run_together it does nothing
        pass


def test_the_barrier_starts_a_round_together():
    naps = ([0.01, 0.6, 0.01], [0.6, 0.01, 0.01], [0.01, 0.01, 0.01])
    jobs = [Sleeper(n) for n in naps]
    main = threading.get_ident()
    assert run_together(jobs, 3, limit=30) == [True, True, True]
    for r in (1, 2):  # nobody begins a round before the slowest is back from the one before
        slowest = max(j.ended[r - 1] for j in jobs)
        assert all(j.began[r] >= slowest for j in jobs), r
        # (and all begin it together: far closer than the 0.6 s by which they would differ without the barrier)
        assert max(j.began[r] for j in jobs) - min(j.began[r] for j in jobs) < 0.3, r
    # set-up, rounds and close of a job ran on one thread, its own
    assert all(len(j.threads) == 1 and j.closed for j in jobs)
    assert len({next(iter(j.threads)) for j in jobs} | {main}) == 4
    # run_alone: the same jobs on the calling thread
    alone = [Sleeper([0.0] * 2) for _ in range(2)]
    run_alone(alone, 2)
    assert all(j.threads == {main} and len(j.began) == 2 and j.closed for j in alone)
