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
import numpy as np
import pytest

from cpprcoder_amd import rcx, workloads
from gpu_support import CODERS, COUNT0, DATA, HEAD, LOW, SHAPES, Damaged, build, check_call, chunk_blocks, context

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
    block = 4096
    nblocks = 2 * 4096 + 900
    d = Damaged(oracle, workloads.by_name(DATA[coder], nblocks * block - 99, 5 + coder), block, coder, 5 + coder)
    cb = chunk_blocks(block, True, nblocks)
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
