"""Several contexts at once, one host thread each (include/rcx.h: a context "is single-threaded; use one context per
thread / stream"; INTEGRATION.md builds the facades' thread_local contexts on that).

Every scenario is a list of jobs for gpu_support.run_together: a job makes its context, its torch.cuda.Stream() and its
guarded buffers on its own thread, and in every round makes its calls and compares what comes back with what the suite
already trusts -- the CPU oracle's streams, the numpy twins of the typed filters and the statistics, zlib.crc32 -- all of
it computed on the main thread before any worker starts.  A kernel that is bit-exact alone is still wrong for a caller
if the bytes, a status or the first bad block differ while another context works, or if a call does not come back.

Each scenario first runs fresh copies of the same jobs one after the other on the main thread (run_alone), so that a
recipe that is wrong without any concurrency fails there, and then asserts that the threaded rounds really overlapped:
a run that serialised by accident proves nothing.  What counts as overlap is the time inside the library alone, from a
call to the return of the synchronisation behind it (gpu_support.library_call): not the filling of guarded buffers in
front of a call, nor the comparisons behind it, which every job does behind the same barrier anyway.  The block counts
are the smallest that keep the calls long enough for that: a 64 KiB block is one serial chain of several milliseconds,
whatever the count of blocks.  LIMIT is a hang guard (run_together ends the session when it is reached), not a
performance figure.

Run as a program (`python tests/test_gpu_threads.py first-question`) this file is the child process of
test_two_threads_ask_the_block_sorts_first_question_at_once: see there.
"""
import ctypes
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import predict_cases as pr
from cpprcoder_amd import predict, rcx, stats, workloads
from gpu_support import (CODERS, DATA, HEAD, Damaged, Guarded, assert_same_blocks, assert_same_items, check_call, chunk_blocks, decode_items,
                         encode_items, gpu_decode, gpu_encode, hip_runtime, jobs_intersect, library_call, oracle_streams, run_alone,
                         run_together)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LIMIT = 120
BLOCK = 65536
N = 48 * BLOCK + 12345            # scenario a: 48 whole blocks and a ragged one
SEEDS = (11, 12, 13)
BIG_BLOCK = 4 * BLOCK             # the growing context's block from round 3 on: 12 whole blocks of N and a ragged one
SMALL = 4096
HOST_N = (2 * 4096 + 900) * SMALL - 99  # the host-buffer pipeline: three chunks of 4 KiB blocks, encode and decode


def test_the_binding_drops_the_gil():
    """ctypes.CDLL releases the GIL around every call, a PyDLL keeps it: with a PyDLL no two threads would ever be inside
    the library at once, and every scenario below would pass for the wrong reason."""
    for lib in (rcx.lib(), stats.lib(), predict.lib()):
        assert isinstance(lib, ctypes.CDLL) and not isinstance(lib, ctypes.PyDLL)


class Job:
    """What every job has: a context and a stream made on its own thread (run_together calls setup there); a round runs
    with the stream as the thread's current one, so that the buffers' copies and the calls all go through it."""

    def setup(self):
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.ctx = rcx.Context(0)
        self.stream = torch.cuda.Stream()

    def __call__(self, r):
        with torch.cuda.stream(self.stream):
            self.round(r)
            self.stream.synchronize()

    def close(self):
        self.ctx.close()


def together(make_jobs, rounds, between=None, **how):
    """The scenario: fresh jobs alone, fresh jobs together -> the share of rounds in which calls of the library on
    different threads overlapped, which must not be 0.  `between` is called between the two."""
    run_alone(make_jobs(), rounds)
    if between is not None:
        between()
    overlapped = run_together(make_jobs(), rounds, LIMIT, calls_only=True, **how)
    share = f"{sum(overlapped)} of {rounds} rounds overlapped"
    print(share)
    assert any(overlapped), "no round ran side by side: " + share
    return overlapped


# ---- a. four device-pointer callers, one per coder ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks_of(oracle):
    """(coder, seed, block) -> (data, slots, sizes), the oracle's; made on demand, on the main thread, and kept."""
    made = {}

    def get(coder, seed, block=BLOCK, n=N):
        key = (coder, seed, block, n)
        if key not in made:
            data = workloads.by_name(DATA[coder], n, seed)
            made[key] = (data,) + tuple(oracle.encode_blocks(data, block, coder=coder, threads=8))
        return made[key]

    return get


class Blocks(Job):
    """encode_blocks_device, sync_status, the oracle's payload and table, decode_blocks_device, the data again: every
    buffer guarded.  `grows`: the context is not reserved ahead, so that its scratch and its divisor table are made inside
    round 0 (ensure_divtab launches on the null stream and synchronises the device), and from round 3 on its blocks are
    256 KiB: the table is built again and the slots are freed and allocated anew, all while the others work."""

    def __init__(self, blocks_of, coder, seeds, grows=False):
        self.coder, self.grows = coder, grows
        self.cases = [blocks_of(coder, s) for s in seeds]
        self.big = [blocks_of(coder, s, BIG_BLOCK) for s in seeds] if grows else None

    def setup(self):
        super().setup()
        if not self.grows:
            self.ctx.reserve(N, BLOCK, self.coder)
        self.held = self.ctx.scratch_bytes()
        assert (self.held == 0) == self.grows

    def round(self, r):
        big = self.grows and r >= 3
        data, slots, sizes = (self.big if big else self.cases)[r % len(self.cases)]
        block = BIG_BLOCK if big else BLOCK
        label = f"coder {self.coder}, round {r}"
        payload, offsets, _ = gpu_encode(self.ctx, data, block, coder=self.coder)
        assert_same_blocks(payload, offsets, slots, sizes, label)
        back, st, _ = gpu_decode(self.ctx, payload, offsets, len(data), block, coder=self.coder)
        assert st == rcx.OK and np.array_equal(back, data), f"{label}: status {st}, round trip"
        if self.grows and r in (0, 3):
            assert self.ctx.scratch_bytes() > self.held, f"{label}: the scratch should have grown in this round"
        elif self.grows:
            assert self.ctx.scratch_bytes() == self.held, label
        self.held = self.ctx.scratch_bytes()


def test_four_coders_on_four_threads(blocks_of):
    def make():
        return [Blocks(blocks_of, coder, SEEDS[k % 3:] + SEEDS[:k % 3], grows=(k == 0)) for k, coder in enumerate(CODERS)]

    assert rcx.block_count(N, BIG_BLOCK) == 13 and N // BIG_BLOCK == 12
    # (13 slots of 256 KiB blocks take more than 49 of 64 KiB blocks: the growing context's slots are allocated anew)
    assert 13 * rcx.block_bound(BIG_BLOCK) > 49 * rcx.block_bound(BLOCK)
    together(make, 6)


# ---- b. four kinds of call at once --------------------------------------------------------------------------------------
def host_cases(oracle):
    """coder -> (data, payload, offsets): HOST_N bytes in 4 KiB blocks, the oracle's compacted streams."""
    made = {}

    def get(coder):
        if coder not in made:
            data = workloads.by_name(DATA[coder], HOST_N, 5 + coder)
            slots, sizes = oracle.encode_blocks(data, SMALL, coder=coder, threads=16)
            made[coder] = (data,) + tuple(oracle.compact(slots, sizes))
        return made[coder]

    return get


@pytest.fixture(scope="module")
def host_case(oracle):
    return host_cases(oracle)


class HostPipeline(Job):
    """rcx_encode_blocks / rcx_decode_blocks in three chunks each (csrc/rcx_host.hpp): work streams, a copy-back stream,
    feeder and drainer threads of the library's own, per context."""

    def __init__(self, case, coder):
        self.coder = coder
        self.data, self.payload, self.offsets = case(coder)
        nblocks = len(self.offsets) - 1
        for decode in (False, True):
            assert -(-nblocks // chunk_blocks(SMALL, decode, nblocks)) == 3

    def round(self, r):
        n = len(self.data)
        dst = np.full(rcx.encode_bound(n, SMALL, self.coder), 0xA5, np.uint8)
        offsets = np.zeros(len(self.offsets), np.uint64)
        with library_call():
            size = self.ctx.encode_blocks_into(self.data, SMALL, dst, offsets, self.coder)
        assert size == len(self.payload) and np.array_equal(offsets, self.offsets), f"coder {self.coder}, round {r}: the table"
        assert np.array_equal(dst[:size], self.payload), f"coder {self.coder}, round {r}: the payload"
        assert bool((dst[size:] == 0xA5).all()), "wrote past the size it reported"
        out = np.full(n + 64, 0x5A, np.uint8)
        with library_call():
            got = self.ctx.decode_blocks_into(self.payload, len(self.payload), self.offsets, SMALL, out[:n], self.coder)
        assert got == n and np.array_equal(out[:n], self.data) and bool((out[n:] == 0x5A).all()), f"coder {self.coder}, round {r}: decode"


class Items(Job):
    """The item calls, whose work tables (itab, itab_host) are the context's: other lengths every round, so that the tables
    are rebuilt; then a shuffled pick with repeats."""

    def __init__(self, oracle, rounds, coder=rcx.CODER_ADAPTIVE):
        self.coder, self.cases = coder, []
        for r in range(rounds):
            rs = np.random.RandomState(300 + r)
            lengths = rs.randint(0, 5001, 300)
            lengths[rs.randint(0, 300, 5)] = 0
            pool = workloads.by_name("zipf", int(lengths.sum()), 40 + r)
            cuts = np.concatenate([[0], np.cumsum(lengths)])
            items = [pool[int(cuts[i]): int(cuts[i + 1])] for i in range(300)]
            pick = np.concatenate([rs.permutation(300)[:150], rs.randint(0, 300, 50)])
            self.cases.append((items, oracle_streams(oracle, items, coder), pick))

    def round(self, r):
        items, want, pick = self.cases[r]
        payload, table = encode_items(self.ctx, items, self.coder)
        assert_same_items(payload, table, want, f"round {r}")
        back, st, _ = decode_items(self.ctx, payload, table, [len(items[i]) for i in pick], self.coder, pick=pick)
        assert st == rcx.OK, (r, st)
        for k, i in enumerate(pick):
            assert np.array_equal(back[k], items[i]), f"round {r}: pick {k} (item {i}) differs"


WIDTH, PLANE_BLOCK, TYPED_N = 8, 4096, 3 * 8 * 4096 + 1001


class TypedChain(Job):
    """One stream, no synchronisation in between: the predictor and plane filter, the block coder, the CRC-32 and the
    statistics of the planes, the decoder, the inverse filter."""

    def __init__(self, oracle, rounds):
        self.cases = []
        for r in range(rounds):
            rs = np.random.RandomState(700 + r)
            walk = np.cumsum(rs.randint(-1000, 1001, TYPED_N // 8)).astype("<i8").view(np.uint8)
            x = np.concatenate([walk, rs.randint(0, 256, TYPED_N - len(walk)).astype(np.uint8)])
            planes = pr.split_numpy(x, WIDTH, PLANE_BLOCK, pr.ZIGZAG)
            slots, sizes = oracle.encode_blocks(planes, SMALL, threads=4)
            cuts = range(0, TYPED_N, SMALL)
            crc = np.array([zlib.crc32(planes[at: at + SMALL].tobytes()) for at in cuts], np.uint32)
            hist = np.stack([np.bincount(planes[at: at + SMALL], minlength=256) for at in cuts]).astype(np.uint32)
            self.cases.append((x, planes, slots, sizes, crc, hist, stats.cost_numpy(hist)))

    def round(self, r):
        x, want_planes, slots, sizes, want_crc, want_hist, want_cost = self.cases[r]
        ctx, n, nblocks = self.ctx, TYPED_N, rcx.block_count(TYPED_N, SMALL)
        src, planes = Guarded(n, 0, x, salt=1), Guarded(n, 0, salt=2)
        dst, table = Guarded(rcx.encode_bound(n, SMALL), 0, salt=3), Guarded(8 * (nblocks + 1), 0, salt=4)
        crc, hist, cost = Guarded(4 * nblocks, 0, salt=5), Guarded(1024 * nblocks, 0, salt=6), Guarded(8 * nblocks, 0, salt=7)
        back, out = Guarded(n, 0, salt=8), Guarded(n, 0, salt=9)
        offs = table.view.view(torch.int64)
        with library_call():
            predict.split_device(ctx, src.view, WIDTH, PLANE_BLOCK, predict.ZIGZAG, planes.view)
            ctx.encode_blocks_device(planes.view, SMALL, dst.view, offs)
            ctx.crc32_blocks_device(planes.view, SMALL, crc.view.view(torch.int32))
            stats.blocks_device(ctx, planes.view, SMALL, hist.view.view(torch.int32), cost.view.view(torch.int64))
            ctx.decode_blocks_device(dst.view, dst.size, offs, n, SMALL, back.view)
            predict.join_device(ctx, back.view, WIDTH, PLANE_BLOCK, predict.ZIGZAG, out.view)
            ctx.sync_status()
        label = f"typed chain, round {r}"
        offsets = offs.cpu().numpy().astype(np.uint64)
        for g, written, what in ((src, 0, "src"), (planes, n, "planes"), (table, 8 * (nblocks + 1), "offsets"), (dst, int(offsets[-1]), "dst"),
                                 (crc, 4 * nblocks, "crc"), (hist, 1024 * nblocks, "hist"), (cost, 8 * nblocks, "cost"), (back, n, "back"),
                                 (out, n, "out")):
            g.check(written, f"{label}: {what}")
        assert np.array_equal(planes.view.cpu().numpy(), want_planes), f"{label}: the planes"
        assert_same_blocks(dst.view[: int(offsets[-1])].cpu().numpy(), offsets, slots, sizes, label)
        assert np.array_equal(crc.view.cpu().numpy().view(np.uint32), want_crc), f"{label}: CRC-32"
        assert np.array_equal(hist.view.cpu().numpy().view(np.uint32).reshape(nblocks, 256), want_hist), f"{label}: counts"
        assert np.array_equal(cost.view.cpu().numpy().view(np.uint64), want_cost), f"{label}: costs"
        assert np.array_equal(back.view.cpu().numpy(), want_planes) and np.array_equal(out.view.cpu().numpy(), x), f"{label}: round trip"


class Resumable(Job):
    """rcx_estream / rcx_dstream in pieces of 4096 bytes: many small launches and blocking copies from one thread."""

    def __init__(self, oracle, rounds, n=200_000, piece=4096):
        self.piece, self.cases = piece, []
        for r in range(rounds):
            data = workloads.zipf(n, 90 + r).tobytes()
            (st, rq), comp, _ = oracle.adaptive_encode(data)
            assert (st, rq) == (0, 0)
            self.cases.append((data, comp))

    def round(self, r):
        data, comp = self.cases[r]
        n, piece = len(data), self.piece
        es = self.ctx.estream(n)
        sink, st, rq = bytearray(n.to_bytes(4, "little")), rcx.PENDING, n
        for at in range(0, n, piece):
            with library_call():
                st, rq, body, tail = es.encode(data[at: at + piece])
            sink += body + tail
            assert (st, rq) == ((rcx.OK, 0) if at + piece >= n else (rcx.PENDING, n - at - piece)), (r, at, st, rq)
        es.close()
        assert bytes(sink) == comp, f"resumable encoder, round {r}"
        ds = self.ctx.dstream()
        out, at, st, rq = b"", 0, rcx.PENDING, 0
        while at < len(comp) and st == rcx.PENDING:
            with library_call():
                st, rq, got = ds.decode(comp[at: at + piece], n)
            at += piece
            out += got
        ds.close()
        assert (st, rq) == (rcx.OK, 0) and out == data, f"resumable decoder, round {r}: status {st}, request {rq}"


def test_four_kinds_of_call_at_once(monkeypatch, oracle, host_case):
    monkeypatch.setenv("RCX_HOST_DEC_CHUNK", "64")  # (below the 16 MiB floor: chunks of the floor, three of them)
    rounds = 4
    items, typed, resumable = Items(oracle, rounds), TypedChain(oracle, rounds), Resumable(oracle, rounds)

    def make():  # (the references are shared; a job's context and stream are made anew in its setup)
        return [HostPipeline(host_case, rcx.CODER_ADAPTIVE), items, typed, resumable]

    together(make, rounds)


# ---- c. two pipelines side by side, and two block sorts ----------------------------------------------------------------------
class BlockSort(Job):
    """rcx_bwt_encode / rcx_bwt_decode on a fresh context; .first is the span of the context's first block-sort call."""

    def __init__(self, oracle, k, rounds, n=5 * 32768 + 77):
        self.cases = []
        for r in range(rounds):
            data = workloads.by_name(("canterbury", "zipf")[k], n, 60 + 10 * k + r)
            self.cases.append((data, oracle.bwt_encode(data)))

    def setup(self):
        super().setup()
        self.first = None

    def round(self, r):
        data, want = self.cases[r]
        start = time.perf_counter()
        with library_call():
            enc = self.ctx.bwt_encode(data)
        self.first = self.first or (start, time.perf_counter())
        assert np.array_equal(enc, want), f"block sort, round {r}"
        with library_call():
            back = self.ctx.bwt_decode(enc)
        assert np.array_equal(back, data), f"inverse block sort, round {r}"


def pipelines_and_sorts(oracle, host_case, rounds):
    """-> (what makes the four jobs, the two block-sort jobs among them)."""
    sorts = [BlockSort(oracle, k, rounds) for k in (0, 1)]
    return (lambda: [HostPipeline(host_case, rcx.CODER_ADAPTIVE), HostPipeline(host_case, rcx.CODER_RANS8)] + sorts), sorts


def test_two_pipelines_and_two_block_sorts(monkeypatch, oracle, host_case):
    """Every stream, mover thread and pinned slot of the host-buffer pipeline twice, next to two block sorts whose
    contexts are fresh: both go through their first block-sort call (rcx_bwt_api.hpp: the kernels' LDS leave) in round
    0.  The ranking is the default one, with ballots."""
    monkeypatch.setenv("RCX_HOST_DEC_CHUNK", "64")
    monkeypatch.delenv("RCX_BWT_MATCH", raising=False)
    make, _ = pipelines_and_sorts(oracle, host_case, 3)
    together(make, 3)


def first_question():
    """The child process of the test below: nothing in this process has asked the question yet."""
    import oracle_lib
    oracle_lib.build_oracle()
    oracle = oracle_lib.oracle()
    assert "RCX_BWT_MATCH" not in os.environ and os.environ["RCX_HOST_DEC_CHUNK"] == "64"
    rounds = 3
    make, sorts = pipelines_and_sorts(oracle, host_cases(oracle), rounds)

    def atomic():  # (no call runs while the environment changes: the jobs' threads do not exist yet)
        os.environ["RCX_BWT_MATCH"] = "atomic"

    def hung(message):
        print(message, flush=True)
        os._exit(3)

    together(make, rounds, between=atomic, stuck=hung)
    (a0, a1), (b0, b1) = (job.first for job in sorts)
    print(f"first block-sort calls: entered {abs(a0 - b0) * 1e3:.3f} ms apart, {(a1 - a0) * 1e3:.3f} ms and {(b1 - b0) * 1e3:.3f} ms long, "
          f"{(min(a1, b1) - max(a0, b0)) * 1e3:.3f} ms side by side")
    assert jobs_intersect([[(a0, a1)], [(b0, b1)]]), "the two contexts' first block-sort calls did not run side by side"
    print("first question ok")


def test_two_threads_ask_the_block_sorts_first_question_at_once():
    """The same scenario under RCX_BWT_MATCH=atomic, in a process of its own.  A context's first block-sort call then
    asks, once per device and process, whether the LDS serves the lanes of one instruction in lane order
    (rcx_bwt_api.hpp: `static int known[64]`, a hipMemset, rcx_bwt_lds_order_k on the null stream, a blocking copy and
    an unsynchronised write of the answer).  In this process the question is long answered -- by the block-sort tests
    that ran before, and at the latest by a pass of the jobs alone -- so two threads can meet there only in a fresh
    process: the child runs the jobs alone with the default ranking, which asks nothing and gives the same bytes, then
    sets RCX_BWT_MATCH=atomic, and then starts the threads, whose contexts are new: the two block sorts' first calls
    leave the same barrier with the question still open.

    What this shows: every byte of both sorts and both pipelines is the oracle's from round 0 on, and the two first
    calls ran side by side (the child asserts that their spans intersect and prints by how much).  What it cannot show:
    that the second thread read known[] before the first wrote it, so that both ran the check -- the library has no
    export that tells, and adding one is not this change's business.  On an MI355X the two threads entered 0.36 ms
    apart into calls of 1.3 and 1.4 ms, side by side for 1.0 ms, and the check takes about 0.3 ms: the second thread may
    have met the open question or the first one's answer.  A run in which it found the answer is the path every other
    block-sort test takes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, RCX_HOST_DEC_CHUNK="64")
    env.pop("RCX_BWT_MATCH", None)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "first-question"], env=env, capture_output=True, text=True, timeout=2 * LIMIT + 120)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the child process of {__name__} is not back after {e.timeout} s; nothing more is started on the GPU", returncode=3)
    print(p.stdout[-3000:])
    if p.returncode not in (0, 1):  # a hang reported by run_together (3), an abort, a fault: no more GPU work behind it
        pytest.exit(f"the child process of {__name__} ended with {p.returncode}: " + p.stdout[-2000:] + p.stderr[-2000:], returncode=3)
    assert p.returncode == 0 and "first question ok" in p.stdout, p.stdout[-3000:] + p.stderr[-4000:]


# ---- d. the status latch belongs to its context -----------------------------------------------------------------------------
class Latch(Job):
    """64 blocks of 4 KiB; in the rounds in which this job is the victim one stream is flipped (the oracle decodes it, to
    other bytes) and one truncated (the oracle runs dry: RCX_E_CORRUPT and that block), in every other round the payload
    is clean: RCX_OK, the data, and no block left to the one-lane kernels."""

    def __init__(self, oracle, k):
        coder, nblocks = CODERS[k], 64
        self.k, self.coder = k, coder
        data = workloads.by_name(DATA[coder], nblocks * SMALL - 99, 20 + k)
        self.clean = Damaged(oracle, data, SMALL, coder, 20 + k)
        d = self.hurt = Damaged(oracle, data, SMALL, coder, 20 + k)
        b, z = 9 + k, len(d.orig[9 + k])
        s = d.padded(b)
        s[HEAD[coder] + 16 + (z - HEAD[coder]) // 2] ^= 0x21
        d.damage(b, "flipped", s)
        d.truncate(30 + k, 5)
        want_st, want_first, want = d.expected()
        assert (want_st, want_first) == (rcx.E_CORRUPT, 30 + k) and b in want and not np.array_equal(want[b], d.good(b))
        assert self.clean.expected()[:2] == (rcx.OK, None)

    def round(self, r):
        label = f"job {self.k}, round {r}"
        if r % 3 == self.k:
            check_call(self.ctx, self.hurt, SMALL, 0, label + " (damaged)")
            return
        payload, offsets = self.clean.streams()
        back, st, _ = gpu_decode(self.ctx, payload, offsets, len(self.clean.data), SMALL, coder=self.coder)
        assert st == rcx.OK and np.array_equal(back, self.clean.data), f"{label}: status {st} next to another context's damaged payload"
        assert self.ctx.last_redo(self.clean.nblocks) == 0, label


def test_a_damaged_payload_is_its_own_contexts(oracle):
    latches = [Latch(oracle, k) for k in range(3)]
    together(lambda: latches, 6)


# ---- e. contexts coming and going -------------------------------------------------------------------------------------------
class ComesAndGoes(Job):
    """Every round: a new context, reserved for 16 blocks of 64 KiB, a round trip against the oracle, and the context
    closed again -- rcx_ctx_destroy synchronises the device and frees a whole context's scratch while the others work."""

    def __init__(self, blocks_of):
        self.cases = [blocks_of(rcx.CODER_ADAPTIVE, s, BLOCK, 15 * BLOCK + 4321) for s in SEEDS]

    def setup(self):
        self.stream = torch.cuda.Stream()

    def round(self, r):
        data, slots, sizes = self.cases[r % len(self.cases)]
        ctx = rcx.Context(0)
        try:
            ctx.reserve(len(data), BLOCK)
            payload, offsets, _ = gpu_encode(ctx, data, BLOCK)
            assert_same_blocks(payload, offsets, slots, sizes, f"context {r}")
            back, st, _ = gpu_decode(ctx, payload, offsets, len(data), BLOCK)
            assert st == rcx.OK and np.array_equal(back, data), f"context {r}: status {st}, round trip"
        finally:
            ctx.close()

    def close(self):
        pass


def test_contexts_come_and_go_while_others_work(blocks_of):
    def make():
        return [ComesAndGoes(blocks_of), Blocks(blocks_of, rcx.CODER_ADAPTIVE, SEEDS), Blocks(blocks_of, rcx.CODER_RANS8, SEEDS[1:] + SEEDS[:1])]

    together(make, 8)


# ---- f. the thread's last HIP error is the thread's --------------------------------------------------------------------------
class LeavesAnError(Blocks):
    """Blocks, but in front of each of its two calls the thread leaves an error behind that nobody reads: a hipFree of
    nonsense through the runtime the library links (tests/test_gpu_host.py does the same on one thread).  The buffers
    exist by then: torch reads the thread's last error too, and would report it as its own."""

    def setup(self):
        super().setup()
        self.hip = hip_runtime()

    def leave_an_error(self):
        assert self.hip.hipFree(ctypes.c_void_p(0x1234)) != 0

    def round(self, r):
        data, slots, sizes = self.cases[r % len(self.cases)]
        payload, offsets, _ = gpu_encode(self.ctx, data, BLOCK, coder=self.coder, before=self.leave_an_error)
        assert_same_blocks(payload, offsets, slots, sizes, f"behind an error, round {r}")
        back, st, _ = gpu_decode(self.ctx, payload, offsets, len(data), BLOCK, coder=self.coder, before=self.leave_an_error)
        assert st == rcx.OK and np.array_equal(back, data), f"behind an error, round {r}: status {st}"


def test_an_error_left_behind_by_one_thread_is_not_another_threads(blocks_of):
    """rcx_enter_device drops the calling thread's pending HIP error and LAUNCHED() reads it behind each launch
    (csrc/rcx_ctx.hpp): right only if that error is per thread.  The thread that leaves errors behind gets RCX_OK and the
    oracle's bytes, and so does the thread next to it, call after call."""
    def make():
        return [LeavesAnError(blocks_of, rcx.CODER_ADAPTIVE, SEEDS), Blocks(blocks_of, rcx.CODER_STATIC, SEEDS)]

    together(make, 4)


if __name__ == "__main__":
    assert sys.argv[1:] == ["first-question"], sys.argv
    first_question()
