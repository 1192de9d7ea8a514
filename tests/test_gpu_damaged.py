"""Damaged streams against the oracle, every coder and launch shape (include/rcx.h, "Damaged streams").

The rule: a block whose stream the reference decodes completely gets the reference's bytes, even when the stream is
damaged (a target past the table, a count edited to 0, flipped payload bytes) or truncated by bytes the reference never
reads; a block whose stream the reference cannot decode (it runs dry -- for the static coder also after a symbol of count
0) makes the call report RCX_E_CORRUPT with the lowest such block; every other block of the call decodes as if alone.  The streams
are the oracle's, damaged on purpose; each damaged one is followed by random bytes so that the oracle does not run dry
on it, and the expected bytes are what the oracle decodes from each stream on its own (test_oracle_golden pins the
oracle to the reference build on damaged streams).  The damage is placed where the kernels' paths part: the first symbol,
in-group positions 0, 1 and 15 of the quad decoders' groups of 16, the last group of the fast loop, the symbol-by-symbol
tail of a ragged last block, runs that drive the synchronous ring refill, and truncated blocks in the middle of a call.
"""
import os

import numpy as np
import pytest

from cpprcoder_amd import rcx, workloads
from test_gpu_parity import gpu_decode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CODERS = (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC, rcx.CODER_RANS, rcx.CODER_RANS8)
HEAD = {0: 5, 1: 516, 2: 1032, 3: 1032}  # bytes in front of the coded payload: header (+ the adaptive coder's 0x00 / table)
LOW = {0: (5, 9), 1: (516, 521)}          # the bytes the first renormalisation shifts in (the static coder skips 516)
SHAPES = {  # launch shapes (read when a context is created, rcx_api.hip rcx_ctx_create) and the output's offset
    "default": ({}, 0),
    "quads16": ({"RCX_DEC_QUADS": "16"}, 0),
    "narrow": ({"RCX_WIDE_WG": "0"}, 0),
    "one_lane": ({"RCX_LANES_PER_BLOCK": "1"}, 0),
    "dst+3": ({}, 3),
}
# per coder; the static coder's bytes use every value, so no count is 0 and its damaged streams decode (see Damaged.damage)
DATA = ("zipf", "uniform", "zipf", "canterbury")
COUNT0 = "past the table onto a count of 0"
KNOBS = ("RCX_DEC_QUADS", "RCX_WIDE_WG", "RCX_LANES_PER_BLOCK", "RCX_ENC_VARIANT", "RCX_ENC_LANES")


def context(env):
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return rcx.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def decode_one(oracle, stream, length, block, coder):
    """The oracle on one block's stream alone -> (ok, bytes)."""
    slots = np.zeros((1, len(stream) + 64), np.uint8)
    slots[0, : len(stream)] = stream
    out, ok = oracle.decode_blocks(slots, np.array([len(stream)], np.uint32), block, length, coder=coder)
    return ok, out


def first_wrong(oracle, stream, good, block, coder):
    ok, out = decode_one(oracle, stream, len(good), block, coder)
    if not ok:
        return None
    diff = np.nonzero(out != good)[0]
    return int(diff[0]) if len(diff) else None


def flip_at_symbol(oracle, stream, size, good, block, coder, targets):
    """A single byte flip in `stream` (`size` bytes of stream, then padding) whose first wrong symbol is one of `targets`
    (a set of symbol indices), found by trying positions around the one that an even spread of the bytes gives."""
    lo = HEAD[coder] + 4
    pay = size - lo
    for want in sorted(targets):
        guess = lo + int(pay * want / max(len(good), 1))
        for p in sorted(range(max(lo, guess - 48), min(len(stream) - 4, guess + 48)), key=lambda q: abs(q - guess)):
            for x in (0x01, 0x80, 0x5A):
                s = stream.copy()
                s[p] ^= x
                if first_wrong(oracle, s, good, block, coder) in targets:
                    return s
    return None


class Damaged:
    """Oracle streams of `data` with some blocks damaged: slots (rows padded as needed), sizes, and per block the kind."""

    def __init__(self, oracle, data, block, coder, seed):
        self.oracle, self.data, self.block, self.coder = oracle, data, block, coder
        self.rs = np.random.RandomState(seed)
        slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=8)
        self.nblocks = len(sizes)
        self.pad = 3 * block
        self.orig = [slots[b, : int(sizes[b])].copy() for b in range(self.nblocks)]
        self.rows = list(self.orig)
        self.kind = {}

    def length(self, b):
        return min(self.block, len(self.data) - b * self.block)

    def good(self, b):
        return self.data[b * self.block: b * self.block + self.length(b)]

    def padded(self, b):
        return np.concatenate([self.orig[b], self.rs.randint(0, 256, self.pad).astype(np.uint8)])

    def damage(self, b, kind, stream, fails=False):
        """fails: the reference cannot decode this stream, padding or not.  That is only the static coder's symbol of count
        0: find() (cpprcoder.h:521-535) never fails -- a target at or past the total falls through to symbol 255 -- but if
        the symbol it gives has count 0, range becomes 0 and the renormalisation (:506-513) runs dry.  Every other damaged
        stream here is padded so that the oracle decodes it completely, and that is checked."""
        ok, _ = decode_one(self.oracle, stream, self.length(b), self.block, self.coder)
        assert ok != fails, f"block {b} ({kind}): the oracle {'decodes' if ok else 'fails on'} it"
        self.rows[b], self.kind[b] = stream, kind

    def restore(self, b):
        self.rows[b] = self.orig[b]
        self.kind.pop(b, None)

    def truncate(self, b, k):
        self.rows[b], self.kind[b] = self.orig[b][:-k], f"truncated by {k}"

    def streams(self):
        sizes = np.array([len(r) for r in self.rows], np.uint64)
        offsets = np.zeros(self.nblocks + 1, np.uint64)
        np.cumsum(sizes, out=offsets[1:])
        return np.concatenate(self.rows), offsets

    def expected(self):
        """-> (status, first bad block or None, {block: expected bytes} for the blocks whose bytes are asserted)"""
        bad, want = [], {}
        for b in range(self.nblocks):
            if b not in self.kind:
                want[b] = self.good(b)
                continue
            ok, out = decode_one(self.oracle, self.rows[b], self.length(b), self.block, self.coder)
            if not ok:
                bad.append(b)
            else:  # (a truncated stream the reference still decodes completely included)
                want[b] = out
        return (rcx.E_CORRUPT if bad else rcx.OK), (bad[0] if bad else None), want


def build(oracle, coder, block, nblocks, seed):
    """About nblocks blocks, the last one ragged; damage of every kind the coder has, in blocks spread over the call."""
    data = workloads.by_name(DATA[coder], (nblocks - 1) * block + block // 4 + 7, seed)
    d = Damaged(oracle, data, block, coder, seed)
    groups = block // 16
    b = 1
    if coder in LOW:
        s = d.padded(b)
        s[LOW[coder][0]: LOW[coder][1]] = 0xFF  # the first target at or past the table
        d.damage(b, "first target past the table", s)
        b += 2
        for name, targets in (("group position 0", {16 * g for g in range(3, 12)}), ("group position 1", {16 * g + 1 for g in range(3, 12)}),
                              ("group position 15", {16 * g + 15 for g in range(3, 12)}),
                              ("last group of the fast loop", set(range(16 * (groups - 1), 16 * groups - 2)))):
            s = flip_at_symbol(oracle, d.padded(b), len(d.orig[b]), d.good(b), block, coder, targets)
            assert s is not None, name
            d.damage(b, name, s)
            b += 2
        for name, fill in (("run of 0xFF", 0xFF), ("run of 0x00", 0x00)):
            s = d.padded(b)
            at = HEAD[coder] + 4 + (len(d.orig[b]) - HEAD[coder]) // 2
            s[at: at + 48] = fill
            d.damage(b, name, s)
            b += 2
    if coder == rcx.CODER_STATIC:
        for name in ("count to 0", "count moved"):
            s = d.padded(b)
            counts = s[4:516].view("<u2").copy()
            used = np.nonzero(counts)[0]
            src, dst = used[len(used) // 2], used[0]
            if name == "count moved":
                counts[dst] = min(int(counts[dst]) + int(counts[src]), 0xFFFF)
            counts[src] = 0
            s[4:516] = counts.view(np.uint8)
            d.damage(b, name, s)
            b += 2
        # the first target past the table, where find() falls through to symbol 255, whose count is now 0: range 0, the
        # reference runs dry whatever follows (cpprcoder.h:500-513), so the call reports RCX_E_CORRUPT for this block
        s = d.padded(b)
        s[4 + 2 * 255: 4 + 2 * 256] = 0
        s[LOW[coder][0]: LOW[coder][1]] = 0xFF
        d.damage(b, COUNT0, s, fails=True)
        b += 2
    if coder in (rcx.CODER_RANS, rcx.CODER_RANS8):
        for i in range(4):
            s = d.padded(b)
            z = len(d.orig[b])
            for _ in range(1 + i):
                s[int(d.rs.randint(HEAD[coder] + 16, z))] ^= int(d.rs.randint(1, 256))
            d.damage(b, f"payload flips ({1 + i})", s)
            b += 2
    last = d.nblocks - 1  # the ragged last block: a flip in its symbol-by-symbol tail
    if coder in LOW:
        n_last = d.length(last)
        s = flip_at_symbol(oracle, d.padded(last), len(d.orig[last]), d.good(last), block, coder, set(range(16 * (n_last // 16), n_last)))
        assert s is not None, "tail flip"
        d.damage(last, "flip in the tail", s)
    return d


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


@pytest.fixture(scope="module")
def contexts():
    cs = {name: context(env) for name, (env, _) in SHAPES.items()}
    yield cs
    for c in cs.values():
        c.close()


@pytest.mark.parametrize("block,nblocks", [(4096, 100), (65536, 24)])
@pytest.mark.parametrize("coder", CODERS)
def test_damaged_blocks_decode_like_the_oracle(contexts, oracle, coder, block, nblocks):
    d = build(oracle, coder, block, nblocks, 100 + coder)
    want_st, want_first, _ = d.expected()
    # only the static coder has damage the reference itself fails on: the symbol of count 0
    if coder == rcx.CODER_STATIC:
        assert want_st == rcx.E_CORRUPT and d.kind[want_first] == COUNT0
    else:
        assert want_st == rcx.OK
    for name, (_, dst_offset) in SHAPES.items():
        check_call(contexts[name], d, block, dst_offset, (name, "payload damage"))
    # then truncated blocks in the middle of the call, their offsets rebuilt (and the count-0 block repaired, so that the
    # lowest failing block is a truncated one).  Which cuts run dry is the oracle's to say, and for these streams it is
    # pinned here: the adaptive decoder does not read the last byte the encoder flushed, so its stream cut by 1 byte still
    # decodes completely and that block's bytes are asserted like any other's; every other cut, and every cut of the
    # static and rANS streams, runs dry: RCX_E_CORRUPT, the lowest such block reported, its bytes not asserted.
    for b in [b for b, k in d.kind.items() if k == COUNT0]:
        d.restore(b)
    cut = dict(zip((d.nblocks // 2 + 2, d.nblocks // 2 + 4, d.nblocks // 2 + 6, d.nblocks // 2 + 8), (1, 4, 5, 16)))
    for b, k in cut.items():
        d.truncate(b, k)
    want_st, want_first, want = d.expected()
    assert {k for b, k in cut.items() if b not in want} == ({4, 5, 16} if coder == rcx.CODER_ADAPTIVE else {1, 4, 5, 16})
    assert want_st == rcx.E_CORRUPT and want_first == min(b for b in cut if b not in want)
    for name, (_, dst_offset) in SHAPES.items():
        check_call(contexts[name], d, block, dst_offset, (name, "truncated"))


@pytest.mark.parametrize("coder", CODERS)
def test_host_buffer_decode_of_damaged_blocks_at_chunk_boundaries(monkeypatch, oracle, coder):
    """rcx_decode_blocks in chunks (RCX_HOST_DEC_CHUNK below the 16 MiB floor: chunks of the floor) against the same
    call with RCX_HOST_SERIAL=1: damaged streams that end a chunk and that start the next one.  A chunk's kernels start
    once its own bytes are on the device, and the decoders read whole 16-byte pieces, up to 15 bytes into the next chunk's
    bytes that may not be there yet: a stream that decodes completely never uses them."""
    import test_gpu_host
    block = 4096
    nblocks = 2 * 4096 + 900
    d = Damaged(oracle, workloads.by_name(DATA[coder], nblocks * block - 99, 5 + coder), block, coder, 5 + coder)
    cb = test_gpu_host.chunk_blocks(block, True, nblocks)
    assert d.nblocks // cb >= 2
    for i, b in enumerate((cb - 1, cb, 2 * cb - 1, 2 * cb)):
        s = d.padded(b)
        z = len(d.orig[b])
        if coder in LOW and i % 2 == 0:
            s[LOW[coder][0]: LOW[coder][1]] = 0xFF
        else:
            s[HEAD[coder] + 16 + (z - HEAD[coder]) // 2] ^= 0x21
        d.damage(b, "chunk boundary", s)
    monkeypatch.setenv("RCX_HOST_DEC_CHUNK", "64")
    ctx = rcx.Context(0)
    try:
        def run(serial):
            if serial:
                monkeypatch.setenv("RCX_HOST_SERIAL", "1")
            else:
                monkeypatch.delenv("RCX_HOST_SERIAL", raising=False)
            payload, offsets = d.streams()
            out = np.zeros(len(d.data) + 64, np.uint8)
            try:
                got = ctx.decode_blocks_into(payload, len(payload), offsets, block, out[: len(d.data)], coder)
                return rcx.OK, out[:got]
            except rcx.RcxError as e:
                return e.status, None

        want_st, _, want = d.expected()
        assert want_st == rcx.OK
        (st_c, chunked), (st_s, serial) = run(False), run(True)
        assert st_c == st_s == rcx.OK and np.array_equal(chunked, serial)
        for b, w in want.items():
            assert np.array_equal(chunked[b * block: b * block + len(w)], w), b
        # the last stream of a chunk truncated, and the first of the next: both calls report it
        for b, k in ((cb - 1, 5), (2 * cb, 1)):
            d.truncate(b, k)
        want_st, _, _ = d.expected()
        assert run(False)[0] == run(True)[0] == want_st == rcx.E_CORRUPT
    finally:
        ctx.close()


def single_stream_cases(oracle, coder):
    """Damaged single streams of a few KiB to about 200 KiB, padded or truncated."""
    rs = np.random.RandomState(60 + coder)
    out = []
    for i, n in enumerate((3000, 20000, 70001, 200000)):
        data = workloads.by_name(("zipf", "uniform", "canterbury", "runs")[i], n, 70 + i)
        if coder == rcx.CODER_ADAPTIVE:
            comp = np.frombuffer(oracle.adaptive_encode(data)[1], np.uint8)
        elif coder == rcx.CODER_STATIC:
            comp = np.frombuffer(oracle.static_encode(data)[1], np.uint8)
        else:
            comp = np.frombuffer(oracle.rans_encode(data, coder == rcx.CODER_RANS8), np.uint8)
        pad = rs.randint(0, 256, n + 4096).astype(np.uint8)
        flipped = np.concatenate([comp, pad])
        for _ in range(3):
            flipped[int(rs.randint(HEAD[coder] + 16, len(comp)))] ^= int(rs.randint(1, 256))
        out += [(n, flipped), (n, comp[: len(comp) - (1, 4, 5, 16)[i]].copy())]
        if coder in LOW:
            s = np.concatenate([comp, pad])
            s[LOW[coder][0]: LOW[coder][1]] = 0xFF
            out.append((n, s))
    return out


@pytest.mark.parametrize("coder", CODERS)
def test_single_streams_decode_like_the_oracle(contexts, oracle, coder):
    """rcx_stream_decode (and for the adaptive coder rcx_dstream_*) on damaged streams: the adaptive coder's
    (status, request_size, bytes) are the oracle's adaptive_decode / adaptive_decode_chunked; the static coder and rANS
    have the bool semantics of include/rcx.h (RCX_OK or RCX_ERROR, and the static coder's symbols before a failure)."""
    ctx = contexts["default"]
    for n, s in single_stream_cases(oracle, coder):
        cap = (n + 15) & ~15
        if coder == rcx.CODER_ADAPTIVE:
            (rst, rrq), rout, _ = oracle.adaptive_decode(s, cap)
            st, rq, out = ctx.stream_decode(s, cap)
            assert (st, rq, out) == (rst, rrq, rout), (n, len(s))
            for piece in (4096, 777):
                (rst, rrq), rout, _ = oracle.adaptive_decode_chunked(s, piece, 1 << 20)
                ds = ctx.dstream()
                got, at, st, rq = b"", 0, rcx.PENDING, 0
                while at < len(s) and st == rcx.PENDING:
                    st, rq, part = ds.decode(s[at: at + piece], 1 << 20)
                    at += piece
                    got += part
                ds.close()
                assert (st, rq, got) == (rst, rrq, rout), (n, len(s), piece)
        elif coder == rcx.CODER_STATIC:
            ok, rout, _ = oracle.static_decode(s, cap)
            st, _, out = ctx.stream_decode(s, cap, coder=coder)
            assert st == (rcx.OK if ok else rcx.ERROR), (n, len(s))
            assert out == rout, (n, len(s))
        else:
            ok, rout = oracle.rans_decode(s, n, simd=coder == rcx.CODER_RANS8)
            st, _, out = ctx.stream_decode(s, n, coder=coder)
            assert st == (rcx.OK if ok else rcx.ERROR), (n, len(s))
            if ok:
                assert out == rout, (n, len(s))
