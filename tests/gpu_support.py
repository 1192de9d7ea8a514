"""What the GPU tests share: the launch-shape knobs and contexts made under them, the `ctx` fixture, guarded buffers and
the device calls wrapped in them, the comparisons with the oracle that most tests make, the launch shapes restated with
the block counts at which they change, damaged streams (built by tests/damaged_cases.py, handed on from here) with the
launch shapes they are decoded under (SHAPES), and run_together: jobs on a host thread each, round by round.

A test file imports what it needs from here (a fixture by name: `from gpu_support import ctx  # noqa: F401`, or
`bwt_ctx as ctx` for the block sort in both rank forms; one context per importing module), never from another test file.  tests/test_support_cpu.py holds Guarded, knobs, chunk_blocks,
shape_edges, the two comparisons and run_together to their contracts on CPU tensors and sleeping jobs.  Nothing here reads /root/reference.
"""
import contextlib
import os
import sys
import threading
import time

import numpy as np
import pytest

import oracle_lib
from cpprcoder_amd import rcx, workloads
# damaged streams live in tests/damaged_cases.py (no torch, so that tests/crafted_cases.py can list them); handed on from here
from damaged_cases import COUNT0, DATA, HEAD, LOW, Damaged, build, first_wrong, flip_at_symbol, oracle_decode_one  # noqa: F401

torch = pytest.importorskip("torch")

CODERS = (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC, rcx.CODER_RANS, rcx.CODER_RANS8)
# the launch-shape variables, read when a context is created (rcx_api.hip rcx_ctx_create)
KNOBS = ("RCX_DEC_QUADS", "RCX_WIDE_WG", "RCX_LANES_PER_BLOCK", "RCX_ENC_VARIANT", "RCX_ENC_LANES")


# ---- the environment and contexts ------------------------------------------------------------------------------------
@contextlib.contextmanager
def knobs(env, clear=()):
    """The environment without the variables in `clear` and with those of `env`; what was there before is back on exit,
    also on an exception."""
    saved = {k: os.environ.get(k) for k in (*clear, *env)}
    try:
        for k in clear:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def context(env=None):
    """A context of the launch shape `env` asks for and no other (the knobs are read at creation)."""
    with knobs(env or {}, clear=KNOBS):
        return rcx.Context(0)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = rcx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["ballot", "atomic"])
def bwt_ctx(request):
    """The block-sort tests' context (`from gpu_support import bwt_ctx as ctx  # noqa: F401`): every test that takes it runs
    in both forms of the counting pass's rank (csrc/rcx_bwt.hpp): with ballots -- the default, documented behaviour only
    -- and with one returning LDS atomic per key, which a caller opts into with RCX_BWT_MATCH=atomic (read at the
    context's first block-sort call, so it stays set while the context lives)."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    with knobs({"RCX_BWT_MATCH": request.param}):
        c = rcx.Context(0)
        yield c
        c.close()


# ---- guarded buffers ---------------------------------------------------------------------------------------------------
GUARD = 256  # bytes of guard pattern on each side of every buffer a device call is handed


class Guarded:
    """A buffer handed to a kernel, as a view into a larger tensor: GUARD bytes, `offset` more, the buffer, GUARD
    bytes.  Everything that is not buffer content holds a position-dependent pattern (nonzero; its complement with
    `invert`), and a copy of the whole tensor is kept, so that a check after the call sees any byte written outside
    the range the call may write, and any byte of an input that the call changed."""

    def __init__(self, size, offset=0, content=None, salt=0, invert=False, device="cuda"):
        self.at = GUARD + offset
        self.size = size
        i = np.arange(self.at + size + GUARD, dtype=np.int64)
        image = ((i * 37 + salt * 101 + 11) % 251 + 1).astype(np.uint8)
        if invert:
            image = ~image
        if content is not None:
            image[self.at: self.at + len(content)] = np.frombuffer(np.ascontiguousarray(content).tobytes(), np.uint8)
        self.tensor = torch.from_numpy(image).to(device)
        self.before = self.tensor.clone()
        self.view = self.tensor[self.at: self.at + size]

    def check(self, written=0, what="buffer"):
        """Nothing changed but the first `written` bytes of the buffer."""
        hi = self.at + written
        for lo_, hi_ in ((0, self.at), (hi, self.tensor.numel())):
            if not torch.equal(self.tensor[lo_:hi_], self.before[lo_:hi_]):
                first = lo_ + int(torch.nonzero(self.tensor[lo_:hi_] != self.before[lo_:hi_])[0, 0])
                raise AssertionError(f"{what}: byte {first - self.at} changed, outside the {written} bytes from 0 it may write")


# ---- the device calls, every buffer guarded ----------------------------------------------------------------------------
_calls = threading.local()  # .spans: where run_together collects the calling thread's library_call() spans of a round


@contextlib.contextmanager
def library_call():
    """Around calls of the library, up to the return of the synchronisation behind them: time.perf_counter() at both
    ends, kept for run_together, whose overlap measure counts only these spans -- not the allocation and filling of the
    guarded buffers in front of a call or the comparisons behind it.  Outside run_together it does nothing."""
    start = time.perf_counter()
    try:
        yield
    finally:
        spans = getattr(_calls, "spans", None)
        if spans is not None:
            spans.append((start, time.perf_counter()))


def run_filter(ctx, call, what, x, src_offset=0, dst_offset=0):
    """One device call of a typed filter, call(src, dst), with both buffers guarded -> the n bytes written; the source is
    unchanged, and nothing but the n bytes of the destination is written.  `what` names the call in a failure."""
    n = len(x)
    src = Guarded(n, src_offset, x, salt=1)
    dst = Guarded(n, dst_offset, salt=2)
    assert n == 0 or (src.view.data_ptr() % 16 == src_offset % 16 and dst.view.data_ptr() % 16 == dst_offset % 16)
    call(src.view, dst.view)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    what = f"{what} n={n} offsets {src_offset}, {dst_offset}"
    src.check(0, what + ": src")
    dst.check(n, what + ": dst")
    return dst.view.cpu().numpy()


def _encode(ctx, data, block, src_offset, coder, dst_offset, invert, before=None):
    """-> (dst, offs, offsets np.uint64): the guarded destination and table after the call and its checks."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = len(data)
    nblocks = rcx.block_count(n, block)
    src = Guarded(n, src_offset, data, salt=1, invert=invert)
    dst = Guarded(rcx.encode_bound(n, block, coder), dst_offset, salt=2, invert=invert)
    offs = Guarded(8 * (nblocks + 1), 0, salt=3, invert=invert)
    with library_call():
        if before is not None:
            before()
        ctx.encode_blocks_device(src.view, block, dst.view, offs.view.view(torch.int64), coder=coder)
        ctx.sync_status()
    offsets = offs.view.view(torch.int64).cpu().numpy().astype(np.uint64)
    src.check(0, "encode src")
    offs.check(8 * (nblocks + 1), "encode offsets")
    dst.check(int(offsets[-1]), "encode dst")
    return dst, offs, offsets


def gpu_encode(ctx, data, block, src_offset=0, coder=0, dst_offset=0, invert=False, before=None):
    """-> (payload np.uint8, offsets np.uint64, the device views) through the device-pointer entry points.  Every buffer is
    guarded (Guarded): the source is not written, and nothing is written past offsets[nblocks] of dst or around the table.
    `before`, if given, is called once the buffers exist, right in front of the library call."""
    dst, offs, offsets = _encode(ctx, data, block, src_offset, coder, dst_offset, invert, before)
    return dst.view[: int(offsets[-1])].cpu().numpy(), offsets, (dst.view, offs.view.view(torch.int64))


def gpu_decode(ctx, payload, offsets, n, block, dst_offset=0, comp_offset=0, coder=0, invert=False, before=None):
    """Decode through the device-pointer entry point -> (out np.uint8, status, first bad block).  The compressed bytes
    and the table are guarded inputs (not written; what lies behind comp_size is the guard pattern, not zeros), and
    nothing is written outside the n output bytes.  `before` as in gpu_encode."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    comp = Guarded(len(payload), comp_offset, payload, salt=4, invert=invert)
    table = np.ascontiguousarray(np.asarray(offsets).astype(np.int64))
    offs = Guarded(8 * len(table), 0, table.view(np.uint8), salt=5, invert=invert)
    out = Guarded(n, dst_offset, salt=6, invert=invert)
    with library_call():
        if before is not None:
            before()
        ctx.decode_blocks_device(comp.view, len(payload), offs.view.view(torch.int64), n, block, out.view, coder=coder)
        st, bad = ctx.sync_status(raise_on_error=False)
    comp.check(0, "decode comp")
    offs.check(0, "decode offsets")
    out.check(n, "decode dst")
    return out.view.cpu().numpy(), st, bad


def round_trip_on_device(ctx, data, block, dst_offset=0):
    """Encode, then decode from the encoder's own device buffers where they lie -> (out np.uint8, status).  The encoder
    writes only the streams and the table, the decoder only its n output bytes, and neither writes its input."""
    n = len(data)
    dst, offs, offsets = _encode(ctx, data, block, 0, 0, 0, False)
    dst.before, offs.before = dst.tensor.clone(), offs.tensor.clone()  # the decoder's inputs: nothing may change now
    out = Guarded(n, dst_offset, salt=6)
    ctx.decode_blocks_device(dst.view, int(offsets[-1]), offs.view.view(torch.int64), n, block, out.view)
    st, _ = ctx.sync_status(raise_on_error=False)
    dst.check(0, "decode comp")
    offs.check(0, "decode offsets")
    out.check(n, "decode dst")
    return out.view.cpu().numpy(), st


def encode_items(ctx, items, coder, src_offset=0, dst_offset=0, invert=False):
    """Through the device call with every buffer guarded -> (payload, comp_offsets): the source is not written, the
    destination only in [0, comp_offsets[nitems]), the table only in its nitems + 1 entries."""
    lengths = [len(x) for x in items]
    soffs = rcx.item_offsets(lengths)
    data = np.concatenate(items) if items else np.zeros(0, np.uint8)
    src = Guarded(len(data), src_offset, data, salt=1, invert=invert)
    dst = Guarded(rcx.encode_items_bound(soffs, coder), dst_offset, salt=2, invert=invert)
    offs = Guarded(8 * len(soffs), 0, salt=3, invert=invert)
    with library_call():
        ctx.encode_items_device(src.view, soffs, dst.view, offs.view.view(torch.int64), coder=coder)
        ctx.sync_status()
    table = offs.view.view(torch.int64).cpu().numpy().astype(np.uint64)
    src.check(0, "encode src")
    offs.check(8 * len(soffs), "encode table")
    dst.check(int(table[-1]), "encode dst")
    return dst.view[: int(table[-1])].cpu().numpy(), table


def decode_items(ctx, payload, comp_offsets, lengths, coder, pick=None, comp_offset=0, dst_offset=0, invert=False):
    """Through the device call, guarded -> (list of the picked items' bytes, status, first bad index).  `lengths` are the
    decoded lengths of the picks."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    comp = Guarded(len(payload), comp_offset, payload, salt=4, invert=invert)
    table = np.ascontiguousarray(np.asarray(comp_offsets).astype(np.int64))
    offs = Guarded(8 * len(table), 0, table.view(np.uint8), salt=5, invert=invert)
    doffs = rcx.item_offsets(lengths)
    n = int(doffs[-1])
    out = Guarded(n, dst_offset, salt=6, invert=invert)
    with library_call():
        ctx.decode_items_device(comp.view, len(payload), offs.view.view(torch.int64), doffs, out.view, pick=pick, coder=coder)
        st, bad = ctx.sync_status(raise_on_error=False)
    comp.check(0, "decode comp")
    offs.check(0, "decode table")
    out.check(n, "decode dst")
    flat = out.view.cpu().numpy()
    return [flat[int(doffs[k]): int(doffs[k + 1])] for k in range(len(lengths))], st, bad


# ---- comparisons with the oracle ---------------------------------------------------------------------------------------
def _tag(label):
    return "" if label is None else f"{label}: "


def assert_same_blocks(payload, offsets, slots, sizes, label=None):
    assert np.array_equal(np.diff(offsets.astype(np.int64)), sizes.astype(np.int64)), f"{_tag(label)}per-block sizes differ"
    for b in range(len(sizes)):
        got = payload[int(offsets[b]): int(offsets[b + 1])]
        assert np.array_equal(got, slots[b, : int(sizes[b])]), f"{_tag(label)}block {b} differs"


def assert_same_items(payload, offsets, want, label=None):
    """`want`: every item's stream, None for an item of length 0 (which has no stream)."""
    table = np.concatenate([[0], np.cumsum([0 if s is None else len(s) for s in want], dtype=np.int64)])
    assert np.array_equal(np.asarray(offsets).astype(np.int64), table), f"{_tag(label)}comp_offsets differ from the oracle's sizes"
    for i, s in enumerate(want):
        got = payload[int(offsets[i]): int(offsets[i + 1])]
        assert s is None or np.array_equal(got, s), f"{_tag(label)}item {i} differs"


def check_blocks(ctx, oracle, data, block, coder=0, src_offset=0, dst_offset=0, comp_offset=0, threads=8, label=None):
    """The oracle encodes, the GPU encodes (the source at src_offset), every block's stream is the oracle's, the GPU decodes
    (from comp_offset, to dst_offset) and the bytes are `data` again -> (payload, offsets)."""
    slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=threads)
    payload, offsets, _ = gpu_encode(ctx, data, block, src_offset=src_offset, coder=coder)
    assert_same_blocks(payload, offsets, slots, sizes, label)
    back, st, _ = gpu_decode(ctx, payload, offsets, len(data), block, dst_offset=dst_offset, comp_offset=comp_offset, coder=coder)
    assert st == 0 and np.array_equal(back, data), f"{_tag(label)}status {st}, round trip"
    return payload, offsets


def check_items(ctx, items, want, coder=0, src_offset=0, dst_offset=0, comp_offset=0, out_offset=0, label=None):
    """The item twin: the GPU encodes `items` (the source at src_offset, the streams to dst_offset), every stream is its
    entry of `want`, the GPU decodes (from comp_offset, to out_offset) and every item is back -> (payload, comp_offsets)."""
    payload, offs = encode_items(ctx, items, coder, src_offset=src_offset, dst_offset=dst_offset)
    assert_same_items(payload, offs, want, label)
    back, st, _ = decode_items(ctx, payload, offs, [len(x) for x in items], coder, comp_offset=comp_offset, dst_offset=out_offset)
    assert st == rcx.OK, f"{_tag(label)}status {st}"
    for i, x in enumerate(items):
        assert np.array_equal(back[i], x), f"{_tag(label)}item {i} ({len(x)} bytes) does not round-trip"
    return payload, offs


def check_golden_blocks(ctx, t, coder):
    """One block table of tests/golden: the input is the one the table was made from, every block's size and fnv1a64 (and
    the total, where the table has one) are the reference's, and the round trip returns the input."""
    label = (t["workload"], t["block"], t["coder"])
    data = workloads.by_name(t["workload"], t["n"], t["seed"])
    assert oracle_lib.sha(data) == t["input_sha256"], label
    payload, offsets, _ = gpu_encode(ctx, data, t["block"], coder=coder)
    assert [int(x) for x in np.diff(offsets.astype(np.int64))] == t["sizes"], label
    fnv = ["%016x" % oracle_lib.fnv1a64(payload[int(offsets[b]): int(offsets[b + 1])]) for b in range(len(t["sizes"]))]
    assert fnv == t["fnv1a64"], label
    if "total" in t:
        assert int(offsets[-1]) == t["total"], label
    back, st, _ = gpu_decode(ctx, payload, offsets, t["n"], t["block"], coder=coder)
    assert st == 0 and np.array_equal(back, data), label


def oracle_streams(oracle, items, coder, threads=16):
    """The reference's stream of every item on its own (None for an item of length 0, which has no stream)."""
    out = [None] * len(items)

    def work(first):
        for i in range(first, len(items), threads):
            if len(items[i]):
                slots, sizes = oracle.encode_blocks(items[i], len(items[i]), coder=coder)
                out[i] = slots[0, : int(sizes[0])].copy()

    pool = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    return out


def chunk_blocks(block, decode, nblocks):
    """csrc/rcx_host.hpp host_chunk_blocks(): how many blocks the host-buffer calls put into a chunk."""
    cb = max(4096 if decode else 2048, -(-(16 << 20) // block))
    while -(-nblocks // cb) > 2048:
        cb *= 2
    chunks = -(-nblocks // cb)
    if chunks > 1:
        cb = -(-nblocks // chunks)
    return (cb + 63) & ~63


# ---- launch shapes by block count (csrc/rcx_launch.hpp) ------------------------------------------------------------------
STATIC_ONE_WAVE = 32768  # blocks from which the static encoder is the one-wave kernel (encode_launches, static3)


def _pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def encode_lanes(nblocks, cus):
    """encode_lanes(): blocks per workgroup of the multi-wave encoders -- the power of two that gives every CU a
    workgroup, 64 at the most."""
    return min(_pow2_at_least(-(-nblocks // cus)), 64)


def decode_quads(nblocks, cus):
    """decode_quads(): blocks per wave of the 4-lane decoders -- the power of two that gives every SIMD (4 a CU) a wave,
    16 at the most."""
    return min(_pow2_at_least(-(-nblocks // (4 * cus))), 16)


SHAPE_EDGE_IDS = tuple(f"{k}cus{d:+d}" if d else f"{k}cus" for k in (1, 2, 4, 8, 16, 32) for d in (-1, 0, 1)) + ("32767", "32768", "32769")


def shape_edges(cus):
    """The block counts at which a launch shape changes on a device of `cus` compute units, and their neighbours: m - 1,
    m, m + 1 for m = cus x 1, 2, 4, ... 32 (encode_lanes doubles behind each; decode_quads behind 4, 8, 16 and 32 cus),
    and 32767 ... 32769 (the static encoder's change of kernel).  One entry per SHAPE_EDGE_IDS, in that order; a count
    is 1 at the least."""
    return [max(k * cus + d, 1) for k in (1, 2, 4, 8, 16, 32) for d in (-1, 0, 1)] + [STATIC_ONE_WAVE - 1, STATIC_ONE_WAVE, STATIC_ONE_WAVE + 1]


# ---- damaged streams (include/rcx.h, "Damaged streams") ----------------------------------------------------------------
SHAPES = {  # launch shapes (read when a context is created, rcx_api.hip rcx_ctx_create) and the output's offset
    "default": ({}, 0),
    "quads16": ({"RCX_DEC_QUADS": "16"}, 0),
    "narrow": ({"RCX_WIDE_WG": "0"}, 0),
    "one_lane": ({"RCX_LANES_PER_BLOCK": "1"}, 0),
    "dst+3": ({}, 3),
}


def check_call(ctx, d, block, dst_offset, label):
    payload, offsets = d.streams()
    n = len(d.data)
    back, st, first = gpu_decode(ctx, payload, offsets, n, block, dst_offset=dst_offset, coder=d.coder)
    want_st, want_first, want = d.expected()
    assert st == want_st, (label, st, want_st)
    if want_first is not None:
        assert first == want_first, (label, first, want_first)
    for b, w in want.items():
        got = back[b * block: b * block + len(w)]
        assert np.array_equal(got, w), (label, b, d.kind.get(b, "undamaged"))


# ---- several contexts at once, one host thread each (tests/test_gpu_threads.py) ------------------------------------------
def jobs_intersect(rows):
    """rows: per job its list of (start, end) spans, None or empty for a job that did not run -> does a span of one job
    intersect a span of another?"""
    spans = sorted((start, end, i) for i, row in enumerate(rows) for start, end in row or ())
    ends = {}  # job -> the latest end of its spans so far
    for start, end, i in spans:
        if any(start < e for j, e in ends.items() if j != i):
            return True
        ends[i] = max(end, ends.get(i, end))
    return False


def stuck_message(where, limit):
    """What ends the session when threads did not come back: `where` = [(job index, what it was doing)]."""
    jobs = ", ".join(f"job {i} ({what})" for i, what in where)
    return (f"run_together: {jobs} not back after {limit} s: a call of the library hangs; nothing more is started on the "
            "GPU in this session")


def _end_the_session(message):
    pytest.exit(message, returncode=3)


def run_together(jobs, rounds, limit, stuck=_end_the_session, calls_only=False):
    """Every job on a host thread of its own, `rounds` rounds, the calls of a round started together -> per round, whether
    the intervals of at least two jobs intersected.  A job's intervals are the library_call() spans it went through in
    the round: the time it spent in the library, from the call to the return of its synchronisation.  A job that went
    through none counts with its whole round; with `calls_only` that is an error of the job instead, so that what the GPU
    tests assert about overlap is never the set-up and the comparisons that all jobs do behind the same barrier.

    A job is a callable job(round) -> None that owns its context, its torch.cuda.Stream() and its guarded buffers.  If it
    has a setup() it makes them there, and a close() frees them: both run on the job's thread too, in front of the first
    round and behind the last.  All threads wait at a threading.Barrier in front of every round, and each takes
    time.perf_counter() around its round.  The first exception of any thread is raised again here, on the calling thread,
    as an AssertionError that names the job's index and the round; the other threads stop at their next barrier.  However
    a thread leaves, a job whose set-up succeeded is closed on that thread, so that no context is left to be destroyed
    (a device synchronisation) whenever and wherever the garbage collector finds it.  Threads
    that are not back `limit` seconds after the start are reported through `stuck` (stuck_message); by default that ends
    the whole pytest session with pytest.exit, because a call that hangs in the library must not be followed by more GPU
    work from later tests (the threads are daemons: they do not keep the process).

    The binding loads the library with ctypes.CDLL, which drops the GIL for the duration of every call (a PyDLL would
    keep it), and so do torch's copies and synchronisations: Python threads do overlap inside the library.  That the
    rounds really ran side by side is what the returned list is for; a test asserts it."""
    count = len(jobs)
    barrier = threading.Barrier(count)
    lock = threading.Lock()
    spans = [[None] * count for _ in range(rounds)]
    doing = ["set-up"] * count
    errors = []  # (job index, what it was doing, the exception), the first one first

    def work(i):
        job, ready = jobs[i], False
        try:
            try:
                if hasattr(job, "setup"):
                    job.setup()
                ready = True
                for r in range(rounds):
                    doing[i] = f"waiting for round {r}"
                    barrier.wait()
                    doing[i] = f"round {r}"
                    calls = _calls.spans = []
                    start = time.perf_counter()
                    job(r)
                    end = time.perf_counter()
                    _calls.spans = None
                    assert calls or not calls_only, "the job went through no library_call() in this round"
                    spans[r][i] = calls or [(start, end)]
            except threading.BrokenBarrierError:
                pass  # another job failed or hangs: this one stops here
            finally:
                _calls.spans = None
                if ready and hasattr(job, "close"):
                    if sys.exc_info()[0] is None:  # (a round's exception keeps the round's name)
                        doing[i] = "closing"
                    job.close()
            doing[i] = None
        except BaseException as e:  # noqa: B036 (whatever it is, it is reported on the calling thread)
            with lock:
                errors.append((i, doing[i], e))
            doing[i] = None
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i,), daemon=True, name=f"run_together-{i}") for i in range(count)]
    deadline = time.monotonic() + limit
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(deadline - time.monotonic(), 0))
    alive = [(i, doing[i]) for i, t in enumerate(threads) if t.is_alive()]
    if alive:
        barrier.abort()
        # (a job that waits at the barrier is kept there by one that is not back from its round: name the latter)
        stuck(stuck_message([w for w in alive if not str(w[1]).startswith("waiting")] or alive, limit))
    if errors:
        i, what, e = errors[0]
        raise AssertionError(f"job {i}, {what}: {type(e).__name__}: {e}") from e
    return [jobs_intersect(row) for row in spans]


def run_alone(jobs, rounds):
    """The same jobs and rounds one after the other on the calling thread: what a scenario does first, so that a recipe
    that is wrong without any concurrency fails here."""
    for i, job in enumerate(jobs):
        try:
            if hasattr(job, "setup"):
                job.setup()
            for r in range(rounds):
                job(r)
            if hasattr(job, "close"):
                job.close()
        except Exception as e:
            raise AssertionError(f"alone: job {i}: {type(e).__name__}: {e}") from e


def hip_runtime():
    """The HIP runtime the library links, as a ctypes handle with hipFree and hipGetLastError declared."""
    import ctypes as C
    rcx.lib()
    path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), None)
    assert path, "the HIP runtime should be loaded by now"
    hip = C.CDLL(path)
    hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
    hip.hipGetLastError.argtypes, hip.hipGetLastError.restype = [], C.c_int
    return hip
