"""The resumable coders (rcx_dstream_*, rcx_estream_*, include/rcx.h) across their call boundaries: the table halving inside
a live object, the decoder's launch loop and its input buffer under a backlog, the encoder's rewind and RCX_E_CAPACITY
contract around a pending run longer than any caller's guess, and several live objects on one context.

Every expected value is the CPU oracle's or a reference-built fixture's (tests/golden/long_streams.json); nothing is derived
from the GPU path's own output.  Where the Python wrappers hide a parameter (dst_cap, the E_CAPACITY retry) the tests call
rcx.lib() themselves; every dst they hand over is exactly dst_cap bytes followed by canary bytes."""
import ctypes as C

import numpy as np
import pytest

import golden_cases
import resumable_cases as rc
import trace_cases
from cpprcoder_amd import rcx, workloads
from gpu_support import ctx, gpu_decode, gpu_encode, assert_same_blocks  # noqa: F401
from oracle_lib import sha

pytestmark = pytest.mark.gpu

CANARY, CANARY_BYTES = 0xA5, 64
NO_LIMIT = (1 << 64) - 1


class Dst:
    """A destination of exactly `cap` bytes with canary bytes behind it.  After every call nothing but the bytes the call
    reported may have changed: not the canary, and not the rest of the buffer either."""

    def __init__(self, cap):
        self.cap = cap
        self.buf = np.full(cap + CANARY_BYTES, CANARY, np.uint8)

    def take(self, got, what):
        assert bool((self.buf[self.cap:] == CANARY).all()), f"{what} wrote past dst_cap = {self.cap}"
        kept = min(got, self.cap)
        assert bool((self.buf[kept: self.cap] == CANARY).all()), f"{what} wrote past the {got} bytes it reported"
        out = self.buf[:kept].tobytes()
        self.buf[:kept] = CANARY
        return out


def _ptr(piece):
    src = np.frombuffer(bytes(piece), np.uint8) if isinstance(piece, (bytes, bytearray)) else np.ascontiguousarray(piece, np.uint8)
    return src, (src.ctypes.data if len(src) else None)


def dec_call(ds, piece, dst):
    """rcx_dstream_decode with `piece` into `dst` (a Dst, or a capacity) -> (status, request_size, the symbols of this call)."""
    if not isinstance(dst, Dst):
        dst = Dst(dst)
    src, p = _ptr(piece)
    got, req = C.c_uint64(), C.c_uint32()
    st = rcx.lib().rcx_dstream_decode(ds._h, p, len(src), dst.buf.ctypes.data, dst.cap, C.byref(got), C.byref(req))
    assert got.value <= dst.cap, (got.value, dst.cap)
    return st, req.value, dst.take(got.value, "rcx_dstream_decode")


def enc_call(es, piece, dst_cap, sink_room=NO_LIMIT):
    """rcx_estream_encode, as it is (no retry) -> (status, request_size, emitted_now, bytes for writeByte, bytes for write)."""
    dst = Dst(dst_cap)
    src, p = _ptr(piece)
    got, tail, req = C.c_uint64(), C.c_uint32(), C.c_uint32()
    st = rcx.lib().rcx_estream_encode(es._h, p, len(src), dst.buf.ctypes.data, dst_cap, sink_room, C.byref(got), C.byref(tail), C.byref(req))
    if st == rcx.E_CAPACITY:
        dst.take(0, "rcx_estream_encode (refusing)")
        return st, req.value, got.value, b"", b""
    out = dst.take(got.value, "rcx_estream_encode")
    body = got.value - tail.value
    return st, req.value, got.value, out[:body], out[body:]


def roomy(piece):
    """Room for any call of the carry input: 3 * size + 8 + the pending run (include/rcx.h), the run bounded by its length + 8."""
    return 3 * len(piece) + 8 + rc.CARRY_RUN + 8


def header(n):
    return n.to_bytes(4, "little")


# ---- A: halving inside the resumable objects -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_uniform(oracle, golden):
    """(input, the reference's stream): the oracle's bytes, held to the size and hash the real reference gave."""
    return _long(oracle, golden, rc.LONG_UNIFORM)


@pytest.fixture(scope="module")
def long_min_zipf(oracle, golden):
    return _long(oracle, golden, rc.LONG_MIN_ZIPF)


def _long(oracle, golden, label):
    g = golden["long"]["adaptive"][label]
    v = golden_cases.LONG_ADAPTIVE[label]()
    assert len(v) == g["n"] and sha(v) == g["input_sha256"], label
    (st, rq), comp, size = oracle.adaptive_encode(v)
    assert (st, rq, size) == (0, 0, g["size"]) and sha(comp) == g["sha256"], label
    return v, comp, g


def test_encoder_halves_its_table_at_a_call_boundary(ctx, oracle, long_uniform):
    """rcx_enc_resume_k through the halving at total = 2^24 (cpprcoder.h:1138), in constant pieces of H / 16 bytes: the
    16th call ends with the halving symbol, and the 17th starts from the halved table and the total that came back from
    RcxEState.  The sink's size after every call is the oracle's, the stream the reference's (size and sha256 of
    tests/golden/long_streams.json).  Measured on an MI355X: 12.3 s (17 calls, 16.8 M symbols on one lane)."""
    v, ref, g = long_uniform
    n = len(v)
    assert rc.H % rc.HALVING_PIECE == 0
    want_sizes = oracle.adaptive_encode_trace(v, rc.HALVING_PIECE)[2]
    es = ctx.estream(n)
    sink, sizes = bytearray(header(n)), [4]
    for piece in rc.split(v, rc.constant(n, rc.HALVING_PIECE)):
        st, rq, body, tail = es.encode(piece)
        sink += body + tail
        sizes.append(len(sink))
        assert (st, rq) == ((rcx.PENDING, n - (len(sizes) - 1) * rc.HALVING_PIECE) if not tail else (rcx.OK, 0))
    es.close()
    assert sizes == want_sizes
    assert len(sink) == g["size"] and sha(sink) == g["sha256"]


def test_encoder_halves_its_table_inside_one_byte_calls(ctx, long_uniform):
    """The same input in calls of [H - 1, 1, 1, the rest] bytes: a boundary right before the halving symbol, a call that is
    nothing but that symbol, and one right after it.  The oracle has no trace for uneven pieces: after every call the bytes
    handed on so far are a prefix of the reference's stream, and the whole is that stream.
    Measured on an MI355X: 12.7 s."""
    v, ref, g = long_uniform
    n = len(v)
    es = ctx.estream(n)
    sink, fed = bytearray(header(n)), 0
    for piece in rc.split(v, rc.around_halving(n)):
        st, rq, body, tail = es.encode(piece)
        fed += len(piece)
        sink += body + tail
        assert ref.startswith(bytes(sink)), f"after {fed} bytes the sink is not a prefix of the reference's stream"
        assert (st, rq) == ((rcx.OK, 0) if fed == n else (rcx.PENDING, n - fed)), fed
    es.close()
    assert len(sink) == g["size"] and sha(sink) == g["sha256"]


def _decode_around_halving(ctx, v, comp):
    n = len(v)
    ds = ctx.dstream()
    out, first = [], True
    for cap in rc.around_halving(n):
        st, rq, got = dec_call(ds, comp if first else b"", cap)
        first = False
        out.append(got)
        made = sum(len(x) for x in out)
        assert len(got) == cap, (cap, len(got))
        assert (st, rq) == ((rcx.OK, 0) if made == n else (rcx.PENDING, n - made)), made
    ds.close()
    assert b"".join(out) == v.tobytes()


def test_decoder_halves_its_table_at_a_call_boundary_uniform(ctx, long_uniform):
    """rcx_dec_resume_k through the halving: the whole stream fed at once with dst_cap = H - 1 (sixteen launches of the chunk
    loop in one call), then size = 0 calls with dst_cap 1 (the halving symbol alone), 1 and the rest.  Every Pending asks
    for declared - produced, the symbols are the input.  Measured on an MI355X: 9.4 s."""
    v, comp, _ = long_uniform
    _decode_around_halving(ctx, v, comp)


def test_decoder_halves_its_table_at_a_call_boundary_min_zipf(ctx, oracle, long_min_zipf):
    """The same on 252 symbols that stay at count 1 through the halving, and that stream once more in pieces of 65 521 bytes
    into a roomy dst: status, request size and bytes are adaptive_decode_chunked's.
    Measured on an MI355X: 17.6 s for the two decodes."""
    v, comp, _ = long_min_zipf
    n = len(v)
    _decode_around_halving(ctx, v, comp)
    (wst, wrq), wout, wsize = oracle.adaptive_decode_chunked(comp, rc.CHUNKED_PIECE, n + 64)
    ds = ctx.dstream()
    dst, out, st, rq = Dst(n + 64), [], rcx.PENDING, 0
    for piece in rc.split(comp, rc.constant(len(comp), rc.CHUNKED_PIECE)):
        st, rq, got = dec_call(ds, piece, dst)
        out.append(got)
        if st != rcx.PENDING:
            break
        assert rq == n - sum(len(x) for x in out)
    ds.close()
    out = b"".join(out)
    assert (st, rq, len(out)) == (wst, wrq, wsize) and out == wout


# ---- B: the decoder's launch loop and input buffer -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_stream(oracle):
    v = rc.loop_input()
    return v.tobytes(), oracle.adaptive_encode(v)[1]


@pytest.mark.parametrize("cap", rc.LOOP_CAPS + (rc.LOOP_ONE_CALL,))
def test_decoder_launch_loop_and_chunk_borders(ctx, loop_stream, cap):
    """rcx_dstream_decode launches once per 2^20 symbols: a dst_cap just below, on and just above a launch's worth, two
    launches' worth, and one call of three launches.  Every call but the last fills dst exactly and asks for what is left."""
    v, comp = loop_stream
    n = len(v)
    ds = ctx.dstream()
    dst, out, made = Dst(cap), [], 0
    st, rq, got = dec_call(ds, comp, dst)
    while True:
        out.append(got)
        made += len(got)
        if made == n:
            break
        assert (st, rq, len(got)) == (rcx.PENDING, n - made, cap), (made, st, rq, len(got))
        st, rq, got = dec_call(ds, b"", dst)
    assert (st, rq) == (rcx.OK, 0)
    assert len(out) == -(-n // cap) and b"".join(out) == v
    assert dec_call(ds, b"", dst) == (rcx.OK, 0, b"")  # done stays done
    ds.close()


@pytest.fixture(scope="module")
def backlog_stream(oracle):
    v = rc.backlog_input()
    return v.tobytes(), oracle.adaptive_encode(v)[1]


def _feed_and_drain(ds, v, comp, pieces, caps, out):
    """Feed `pieces` with dst_cap from `caps` in turn, then drain with size = 0; every call is held to the contract."""
    n = len(v)
    made = sum(len(x) for x in out)
    st = rcx.PENDING
    for k, piece in enumerate(pieces):
        cap = caps[k % len(caps)]
        st, rq, got = dec_call(ds, piece, cap)
        out.append(got)
        made += len(got)
        # (the unread backlog is far larger than what these calls take: each fills its dst)
        assert (st, rq, len(got)) == (rcx.PENDING, n - made, cap), (k, st, rq, len(got))
    drain = Dst(rc.DRAIN_CAP)
    while st == rcx.PENDING:
        st, rq, got = dec_call(ds, b"", drain)
        out.append(got)
        made += len(got)
        assert (st, rq) == ((rcx.OK, 0) if made == n else (rcx.PENDING, n - made))
        assert len(got) == rc.DRAIN_CAP or made == n
    assert st == rcx.OK and b"".join(out) == v


def test_decoder_keeps_a_backlog_through_its_buffer_growth(ctx, backlog_stream):
    """Pieces of 100 000 bytes while dst takes 1000 symbols a call: the unread bytes (hundreds of KiB in the end) must survive
    the first buffer of 64 KiB and two doublings, each a copy to a new buffer and a new in_base."""
    v, comp = backlog_stream
    ds = ctx.dstream()
    _feed_and_drain(ds, v, comp, rc.split(comp, rc.constant(len(comp), rc.BACKLOG_PIECE)), (rc.BACKLOG_CAP,), [])
    ds.close()


def test_decoder_backlog_with_uneven_pieces_and_no_room(ctx, backlog_stream):
    """Pieces of 100 000, 1, 1, 70 000, 8 bytes and the rest, dst_cap in turn 0, 1 and 4096: a call with new bytes and no room
    returns Pending, produces nothing and loses nothing."""
    v, comp = backlog_stream
    ds = ctx.dstream()
    _feed_and_drain(ds, v, comp, rc.split(comp, rc.uneven(len(comp))), rc.UNEVEN_CAPS, [])
    ds.close()


def test_decoder_short_first_piece_then_a_backlog(ctx, backlog_stream):
    """A first call of 7 bytes keeps nothing and asks for 8 (cpprcoder.h:877-880); the same bytes come again at the head of a
    100 000-byte piece, and the backlog grows from there."""
    v, comp = backlog_stream
    ds = ctx.dstream()
    assert dec_call(ds, comp[:7], rc.BACKLOG_CAP) == (rcx.PENDING, 8, b"")
    _feed_and_drain(ds, v, comp, rc.split(comp, rc.constant(len(comp), rc.BACKLOG_PIECE)), (rc.BACKLOG_CAP,), [])
    ds.close()


# ---- C: the encoder's rewind and its capacity contract -------------------------------------------------------------------
@pytest.fixture(scope="module")
def carry(oracle):
    """The carry input, the oracle's trace of it in pieces of 64, and the call whose piece ends the run (the jump)."""
    data = rc.carry_input()
    (st, rq), sink, sizes = oracle.adaptive_encode_trace(data, rc.CARRY_PIECE)
    jump = int(np.argmax(np.diff(sizes)))
    assert sizes[jump + 1] - sizes[jump] > rc.FACADE_ROOM
    assert (st, rq) == (0, 0) and sink == oracle.adaptive_encode(data)[1]
    return data.tobytes(), sink, sizes, jump


def test_encoder_capacity_refusal_and_repeat(ctx, carry):
    """dst_cap = 3 * 64 + 4096, the facade's guess: exactly one call, the one that carries through the run of 5000 pending
    bytes, returns RCX_E_CAPACITY with the size needed in *emitted_now and writes nothing; after rcx_estream_rewind the same
    piece with that capacity succeeds.  Sink sizes and stream are the oracle's."""
    data, want, want_sizes, jump = carry
    n = len(data)
    es = ctx.estream(n)
    sink, sizes, refused = bytearray(header(n)), [4], []
    for k, piece in enumerate(rc.split(data, rc.constant(n, rc.CARRY_PIECE))):
        st, rq, emitted, body, tail = enc_call(es, piece, rc.FACADE_ROOM)
        if st == rcx.E_CAPACITY:
            refused.append(k)
            assert emitted == want_sizes[k + 1] - want_sizes[k], emitted
            assert rcx.lib().rcx_estream_rewind(es._h) == rcx.OK
            st, rq, emitted, body, tail = enc_call(es, piece, emitted)
        last = k == n // rc.CARRY_PIECE - 1
        assert (st, rq, len(tail)) == ((rcx.OK, 0, 4) if last else (rcx.PENDING, n - (k + 1) * rc.CARRY_PIECE, 0)), k
        sink += body + tail
        sizes.append(len(sink))
    es.close()
    assert refused == [jump]
    assert sizes == want_sizes and bytes(sink) == want


def _encode_pieces(es, pieces, sink):
    for piece in pieces:
        st, rq, emitted, body, tail = enc_call(es, piece, roomy(piece))
        assert st in (rcx.OK, rcx.PENDING), st
        sink += body + tail
    return st


def test_encoder_rewind_of_the_carrying_call(ctx, oracle, carry):
    """The call whose carry turns the 5000 pending 0xFF bytes in the object's memory into 0x00 is taken back, and a piece that
    ends the run with a smaller byte follows: the stream must be the oracle's for the altered input, 5000 bytes of 0xFF
    included (a rewind that forgot them would leave 0x00).  Then the mirror: the piece without the carry is taken back and
    the carrying one follows."""
    data, want, _, jump = carry
    n = len(data)
    altered = rc.without_the_carry(np.frombuffer(data, np.uint8))[0].tobytes()
    at = jump * rc.CARRY_PIECE
    assert altered[:at] == data[:at] and altered[at: at + rc.CARRY_PIECE] != data[at: at + rc.CARRY_PIECE]
    want_altered = oracle.adaptive_encode(altered)[1]
    assert b"\xff" * rc.CARRY_RUN in want_altered and b"\xff" * rc.CARRY_RUN not in want
    for first, then, expect in ((data, altered, want_altered), (altered, data, want)):
        es = ctx.estream(n)
        sink = bytearray(header(n))
        _encode_pieces(es, rc.split(first[:at], rc.constant(at, rc.CARRY_PIECE)), sink)
        before = bytes(sink)
        st, rq, emitted, body, tail = enc_call(es, first[at: at + rc.CARRY_PIECE], roomy(first[:rc.CARRY_PIECE]))
        assert st == rcx.PENDING and emitted > rc.CARRY_RUN  # (handed to nobody: the call is taken back)
        assert rcx.lib().rcx_estream_rewind(es._h) == rcx.OK
        rest = then[at:]
        assert _encode_pieces(es, rc.split(rest, rc.constant(len(rest), rc.CARRY_PIECE)), sink) == rcx.OK
        es.close()
        assert bytes(sink[: len(before)]) == before and bytes(sink) == expect


def test_encoder_rewinds_at_the_ends(ctx, oracle):
    """A rewind of an object's first call (RcxEState.started back to 0) before a different first piece; a rewind of the
    finishing call, with unlimited room and with a sink in which only finish() fails (cpprcoder.h:716); and the refusals:
    no call to take back, two rewinds in a row."""
    lib = rcx.lib()
    x = workloads.zipf(6000, 7).tobytes()
    other = workloads.uniform(2000, 8).tobytes()
    n = len(x)
    es = ctx.estream(n)
    assert lib.rcx_estream_rewind(es._h) == rcx.E_ARG  # nothing to take back
    st, rq, emitted, body, tail = enc_call(es, other, 3 * len(other) + 64)
    assert (st, rq) == (rcx.PENDING, n - 2000)
    assert lib.rcx_estream_rewind(es._h) == rcx.OK
    assert lib.rcx_estream_rewind(es._h) == rcx.E_ARG  # a second one in a row
    sink = bytearray(header(n))
    for piece in (x[:2000], x[2000:4000]):
        st, rq, emitted, body, tail = enc_call(es, piece, 3 * len(piece) + 64)
        sink += body + tail
    # the finishing call, taken back and made again
    results = []
    for again in (False, True):
        results.append(enc_call(es, x[4000:], 3 * 2000 + 64))
        if not again:
            assert lib.rcx_estream_rewind(es._h) == rcx.OK
            assert lib.rcx_estream_rewind(es._h) == rcx.E_ARG
    assert results[0] == results[1] and results[1][0] == rcx.OK and len(results[1][4]) == 4
    sink += results[1][3] + results[1][4]
    assert bytes(sink) == oracle.adaptive_encode(x)[1]
    es.close()
    # only finish() finds the sink full
    name, data, piece, cap = [c for c in trace_cases.cases() if c[0] == "uniform, only finish() finds the sink full"][0]
    (wst, wrq), want, want_sizes = oracle.adaptive_encode_trace(data, piece, cap)
    full_cap = (cap + 15) // 16 * 16  # a MemoryStream rounds its capacity up (cpprcoder.h:975)
    n = len(data)
    es = ctx.estream(n)
    sink, sizes = bytearray(header(n)), [4]
    pieces = rc.split(data, rc.constant(n, piece))
    for k, pc in enumerate(pieces):
        room = full_cap - len(sink)
        r = enc_call(es, pc, 3 * len(pc) + 64, room)
        if k == len(pieces) - 1:
            assert lib.rcx_estream_rewind(es._h) == rcx.OK
            assert enc_call(es, pc, 3 * len(pc) + 64, room) == r
            assert (r[0], r[1], r[4]) == (rcx.OK, 0, b"")  # finish() gave up, encode() says Success
        sink += r[3] + r[4]
        sizes.append(len(sink))
    es.close()
    assert (r[0], r[1]) == (wst, wrq) and sizes == want_sizes and bytes(sink)[:cap] == want


# ---- E: several objects on one context -----------------------------------------------------------------------------------
def test_several_live_objects_and_block_calls_on_one_context(ctx, oracle):
    """Two decoders and two encoders advance round-robin on one context, each with its own input and piece size, and between
    the rounds the context codes 8 blocks of 4096 bytes: no object's state, input buffer or slot is another's, and none is
    the context's scratch.  Every stream, every decoded buffer and every block is the oracle's."""
    inputs = rc.interleaved_inputs()
    jobs = []
    for kind, v, piece in inputs:
        comp = oracle.adaptive_encode(v)[1]
        if kind == "dec":
            jobs.append({"kind": kind, "obj": ctx.dstream(), "feed": rc.split(comp, rc.constant(len(comp), piece)), "want": v, "got": bytearray(), "n": len(v)})
        else:
            jobs.append({"kind": kind, "obj": ctx.estream(len(v)), "feed": rc.split(v, rc.constant(len(v), piece)), "want": comp, "got": bytearray(header(len(v))),
                         "n": len(v)})
    rounds = max(len(j["feed"]) for j in jobs)
    blocks = workloads.zipf(rc.BLOCKS * rc.BLOCK, 99)
    slots, sizes = oracle.encode_blocks(blocks, rc.BLOCK)
    for r in range(rounds):
        for j in jobs:
            if r >= len(j["feed"]):
                continue
            last = r == len(j["feed"]) - 1
            if j["kind"] == "dec":
                st, rq, got = dec_call(j["obj"], j["feed"][r], 1 << 17)
                j["got"] += got
                assert (st, rq) == ((rcx.OK, 0) if last else (rcx.PENDING, j["n"] - len(j["got"]))), (r, st, rq)
            else:
                st, rq, emitted, body, tail = enc_call(j["obj"], j["feed"][r], 3 * len(j["feed"][r]) + 64)
                j["got"] += body + tail
                assert st == (rcx.OK if last else rcx.PENDING), (r, st)
            assert j["want"].startswith(bytes(j["got"])), (r, j["kind"])
        if r % 3 == 0:
            payload, offsets, _ = gpu_encode(ctx, blocks, rc.BLOCK)
            assert_same_blocks(payload, offsets, slots, sizes, f"round {r}")
            back, st, _ = gpu_decode(ctx, payload, offsets, len(blocks), rc.BLOCK)
            assert st == 0 and np.array_equal(back, blocks), r
    for j in jobs:
        assert bytes(j["got"]) == j["want"], j["kind"]
    for k in (2, 0, 3, 1):  # not the order they were made in
        jobs[k]["obj"].close()
