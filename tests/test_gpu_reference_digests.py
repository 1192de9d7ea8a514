"""The kernels held to the reference build directly, on the crafted inputs (tests/crafted_cases.py): every result a device
call can rebuild -- an encode's stream, a decode's (every symbol came out, bytes), a single stream's (status, request size,
bytes) -- has the digest that the real reference build's result has in tests/golden/reference_crafted.json.  The other GPU
tests compare the kernels with the oracle and tests/test_oracle_crafted.py the oracle with these digests; a misreading of
the reference that the oracle and a kernel share passes both and fails here.  Nothing here reads /root/reference or needs
oracle/_ref; the oracle serves only where crafted_cases builds a damaged stream from a valid one.

Status, as include/rcx.h states it ("Damaged streams") and tests/test_gpu_damaged.py maps it: a block or item call whose
streams the reference all decodes completely is RCX_OK and every block has the reference's bytes; a stream the reference
cannot decode makes the call RCX_E_CORRUPT with the lowest such index, the other blocks decode as if alone.  Which streams
those are is read from the fixture: their digest is that of (False, b"").  Every device buffer is guarded
(gpu_support.Guarded); the single-stream calls take host memory, which stands between canary bytes here (Host).

Stored keys that no call of this file rebuilds, all of them (test_every_stored_key_is_accounted_for holds the list to the
fixture):
  * the three encodes past RCX_MAX_BLOCK, which are no block and no item and take a single lane 9 - 12 s each: the two long
    halving inputs, which tests/test_gpu_resumable.py holds to the reference's size and sha256 (golden/long_streams.json),
    and static_cases.natural_stream(), whose stream tests/test_gpu_static_totals.py holds to this fixture's digest;
  * what the reference says beyond a device call's result: the carry family's capped sinks and pieces of 64 ("cap=",
    "chunked piece=64": the sink's bytes when it fills, which the block and item calls have no notion of), the halving
    family's encodes in pieces ("encode chunked": rcx_estream_* hands on bytes call by call, tests/test_gpu_resumable.py
    compares them with the oracle's trace), and the two long halving streams decoded in pieces of 65 521 bytes (17 s on one
    lane; tests/test_gpu_resumable.py does it against the oracle).  The short halving streams and the truncations in
    pieces ARE rebuilt here, through rcx_dstream_*.
"""
import ctypes as C

import numpy as np
import pytest

import agreement_cases
import crafted_cases
import resumable_cases
from agreement_cases import digest
from bwt_cases import BLOCK as BWT_BLOCK
from bwt_cases import ENCODED as BWT_ENCODED
from cpprcoder_amd import rcx
from gpu_support import SHAPES, Guarded, context, decode_items, encode_items, gpu_decode, gpu_encode
from gpu_support import bwt_ctx  # noqa: F401  (both rank forms)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CODERS = (0, 1, 2, 3)
FAILS = digest((False, b""))
MAX_BLOCK, MIN_BLOCK = (1 << 24) - 256, 16   # include/rcx.h RCX_MAX_BLOCK, RCX_MIN_BLOCK
ENCODE_FAMILIES = ("carry", "static", "rans", "adaptive", "halving")
DECODE_FAMILIES = ("static", "rans", "adaptive", "damaged", "truncations")
# encodes past RCX_MAX_BLOCK: see the module's text
LEFT_TO_OTHER_TESTS = {f"halving/{label}/adaptive/encode" for label in crafted_cases.LONG} | {crafted_cases.NATURAL_STREAM + "/static/encode"}


@pytest.fixture(scope="module")
def contexts():
    cs = {name: context(env) for name, (env, _) in SHAPES.items()}
    yield cs
    for c in cs.values():
        c.close()


def of(family, kind):
    return [c for c in crafted_cases.cases(family) if c.kind == kind and c.coder in CODERS]


def check(stored, bad, c, result):
    if digest(result) != stored[crafted_cases.case_key(c)]:
        bad.append(crafted_cases.case_key(c))


# ---- encode keys ----------------------------------------------------------------------------------------------------------
def encodes(family):
    return [c for c in crafted_cases.encodes(family) if c.coder in CODERS and c.n <= MAX_BLOCK]


@pytest.mark.parametrize("family", ENCODE_FAMILIES)
def test_encodes_by_the_item_call(contexts, family):
    """One item call per coder: cases of differing lengths share waves."""
    stored, bad, seen = agreement_cases.stored_crafted(family), [], 0
    for coder in CODERS:
        cases = [c for c in encodes(family) if c.coder == coder]
        if not cases:
            continue
        payload, table = encode_items(contexts["default"], [c.data for c in cases], coder)
        for i, c in enumerate(cases):
            check(stored, bad, c, (payload[int(table[i]): int(table[i + 1])].tobytes(),))
        seen += len(cases)
    assert seen and not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("family", ENCODE_FAMILIES)
def test_encodes_by_the_block_call(contexts, family):
    """The block equal to the case's length, where that is a legal block; cases of one length and coder in one call."""
    stored, bad, seen = agreement_cases.stored_crafted(family), [], 0
    calls = {}
    for c in encodes(family):
        if MIN_BLOCK <= c.n:
            calls.setdefault((c.coder, c.n), []).append(c)
    for (coder, n), cases in calls.items():
        payload, offsets, _ = gpu_encode(contexts["default"], np.concatenate([c.data for c in cases]), n, coder=coder)
        for i, c in enumerate(cases):
            check(stored, bad, c, (payload[int(offsets[i]): int(offsets[i + 1])].tobytes(),))
        seen += len(cases)
    assert seen and not bad, (len(bad), bad[:8])


# ---- decode keys ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decodes():
    """family -> its decode cases, made once in front of the decode tests: the static family's streams take the oracle some
    9 s on the host (tests/test_gpu_static_totals.py, which comes later, shares them), which is then no test's own time."""
    return {family: of(family, "decode") for family in DECODE_FAMILIES}


def joined(streams):
    offsets = np.zeros(len(streams) + 1, np.uint64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    return np.concatenate(streams), offsets


def check_decoded(stored, bad, cases, st, first, outputs, label):
    """One call's status and bytes against the fixture: the cases the reference fails on make it RCX_E_CORRUPT, the lowest
    one reported and their bytes left alone; every other case has the reference's bytes."""
    failing = [i for i, c in enumerate(cases) if stored[crafted_cases.case_key(c)] == FAILS]
    assert st == (rcx.E_CORRUPT if failing else rcx.OK), (label, st, len(failing))
    assert not failing or first == failing[0], (label, first, failing[0])
    for i, c in enumerate(cases):
        if i not in failing:
            check(stored, bad, c, (True, outputs[i].tobytes()))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", DECODE_FAMILIES)
def test_decodes_by_the_block_call(contexts, decodes, family, shape):
    """Cases of one length and coder in one call (64 at the most: a table of static_cases.crafted_blocks), their streams
    (and what is behind the damaged ones) back to back.  Lengths below RCX_MIN_BLOCK are no block: the item call has them."""
    stored, bad, seen = agreement_cases.stored_crafted(family), [], 0
    calls = {}
    for c in decodes[family]:
        if c.n >= MIN_BLOCK:
            calls.setdefault((c.coder, c.n), []).append(c)
    for (coder, n), every in calls.items():
        for at in range(0, len(every), 64):
            cases = every[at: at + 64]
            payload, offsets = joined([c.data for c in cases])
            back, st, first = gpu_decode(contexts[shape], payload, offsets, n * len(cases), n, dst_offset=SHAPES[shape][1], coder=coder)
            check_decoded(stored, bad, cases, st, first, [back[i * n: (i + 1) * n] for i in range(len(cases))], (family, shape, coder, n, at))
            seen += len(cases)
    assert seen and not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", DECODE_FAMILIES)
def test_decodes_by_the_item_call(contexts, decodes, family, shape):
    """One item call per coder, every length in it.  (The static family's crafted streams, 96 MiB of output, take the item
    call under the default shape alone; under every shape they take the block call above.)"""
    stored, bad, seen = agreement_cases.stored_crafted(family), [], 0
    for coder in CODERS:
        cases = [c for c in decodes[family] if c.coder == coder and (shape == "default" or "/crafted/" not in c.key)]
        for at in range(0, len(cases), 64):
            part = cases[at: at + 64]
            payload, offsets = joined([c.data for c in part])
            outputs, st, first = decode_items(contexts[shape], payload, offsets, [c.n for c in part], coder, dst_offset=SHAPES[shape][1])
            check_decoded(stored, bad, part, st, first, outputs, (family, shape, coder, at))
            seen += len(part)
    assert seen and not bad, (len(bad), bad[:8])


# ---- single streams: the truncations and the halving ------------------------------------------------------------------------
class Host:
    """Host memory handed to a single-stream call: 64 canary bytes, the buffer, 64 canary bytes.  check(written): nothing
    changed but the buffer's first `written` bytes (none of it, for a source)."""
    CANARY, EDGE = 0xA5, 64

    def __init__(self, size, content=None):
        self.size = size
        self.all = np.full(size + 2 * self.EDGE, self.CANARY, np.uint8)
        if content is not None:
            self.all[self.EDGE: self.EDGE + size] = np.frombuffer(bytes(content), np.uint8)
        self.before = self.all.copy()
        self.buf = self.all[self.EDGE: self.EDGE + size]
        self.ptr = self.all.ctypes.data + self.EDGE

    def check(self, written, what):
        at = self.EDGE + written
        assert np.array_equal(self.all[: self.EDGE], self.before[: self.EDGE]) and np.array_equal(self.all[at:], self.before[at:]), \
            f"{what}: a byte outside the {written} it may write changed"


def stream_decode(ctx, comp, cap):
    """rcx_stream_decode between canaries -> (status, request size, bytes)."""
    src, dst = Host(len(comp), comp), Host(max(cap, 16))
    size, req = C.c_uint64(), C.c_uint32()
    st = rcx.lib().rcx_stream_decode(ctx._h, rcx.CODER_ADAPTIVE, src.ptr, len(comp), dst.ptr, cap, C.byref(size), C.byref(req))
    assert size.value <= cap
    src.check(0, "rcx_stream_decode src")
    dst.check(size.value, "rcx_stream_decode dst")
    return st, req.value, dst.buf[: size.value].tobytes()


def in_pieces(ctx, c, piece, room):
    """rcx_dstream_* fed `piece` bytes a call, every piece and the destination between canaries -> ((status, request size),
    bytes, their count): adaptive_decode_chunked's tuple."""
    ds = ctx.dstream()
    dst = Host(room)
    out, at, st, req, got = b"", 0, rcx.PENDING, C.c_uint32(), C.c_uint64()
    while at < len(c.data) and st == rcx.PENDING:
        src = Host(len(c.data[at: at + piece]), c.data[at: at + piece])
        dst.before[:] = dst.all
        st = rcx.lib().rcx_dstream_decode(ds._h, src.ptr, src.size, dst.ptr, room, C.byref(got), C.byref(req))
        assert got.value <= room
        src.check(0, "rcx_dstream_decode src")
        dst.check(got.value, "rcx_dstream_decode dst")
        at += piece
        out += dst.buf[: got.value].tobytes()
    ds.close()
    return (st, req.value), out, len(out)


def test_truncated_single_streams(contexts):
    """rcx_stream_decode into the bounded sink, and rcx_dstream_* in pieces into a roomy one: status, request size and bytes
    are what the reference's bounded MemoryStream answers."""
    stored, bad = agreement_cases.stored_crafted("truncations"), []
    cases = [c for c in crafted_cases.cases("truncations") if c.kind == "stream_decode"]
    assert len(cases) == 8
    for c in cases:
        key = crafted_cases.case_key(c)
        check(stored, bad, c, stream_decode(contexts["default"], c.data, c.n))
        for piece in agreement_cases.TRUNCATION_PIECES:
            if digest(in_pieces(contexts["default"], c, piece, 1 << 20)) != stored[f"{key} chunked piece={piece}"]:
                bad.append(f"{key} chunked piece={piece}")
    assert not bad, bad


HALVING = list(crafted_cases.LONG) + ["loop_input", "backlog_input", "carry_input"]


@pytest.mark.parametrize("label", HALVING)
def test_halving_single_streams(contexts, label):
    """rcx_stream_decode of the whole stream (for the two long ones through the halving at total = 2^24, on one lane: some
    ten seconds each, the two streams tests/test_gpu_resumable.py affords); the three short ones also through
    rcx_dstream_* in pieces that fall nowhere in particular."""
    stored, bad = agreement_cases.stored_crafted("halving"), []
    (c,) = [c for c in crafted_cases.cases("halving") if c.kind == "stream_decode" and c.key == f"halving/{label}"]
    check(stored, bad, c, stream_decode(contexts["default"], c.data, c.n))
    if label not in crafted_cases.LONG:
        piece = resumable_cases.CHUNKED_PIECE
        if digest(in_pieces(contexts["default"], c, piece, c.n)) != stored[f"{crafted_cases.case_key(c)} chunked piece={piece}"]:
            bad.append(f"{label} chunked")
    assert not bad, bad


# ---- the block sort -----------------------------------------------------------------------------------------------------------
def test_block_sort(bwt_ctx):  # noqa: F811
    """rcx_bwt_encode_device over every forward block in one call, rcx_bwt_decode_device over those encodings (the GPU's own,
    which the digests have just shown to be the reference's) and over every block of tests/bwt_inverse_cases.py."""
    stored, bad = agreement_cases.stored_crafted("bwt"), []
    cases = list(crafted_cases.bwt(encoded=False))
    enc = [c for c in cases if c.kind == "encode"]
    src = Guarded(BWT_BLOCK * len(enc), 0, np.concatenate([c.data for c in enc]), salt=1)
    dst = Guarded(BWT_ENCODED * len(enc), 0, salt=2)
    bwt_ctx.bwt_encode_device(src.view, dst.view)
    bwt_ctx.sync_status()
    src.check(0, "encode src")
    dst.check(BWT_ENCODED * len(enc), "encode dst")
    made = dst.view.cpu().numpy()
    for i, c in enumerate(enc):
        check(stored, bad, c, (made[i * BWT_ENCODED: (i + 1) * BWT_ENCODED].tobytes(),))
    assert not bad, (len(bad), bad[:8])
    dec = [crafted_cases.Case(c.key, "bwt", "decode", made[i * BWT_ENCODED: (i + 1) * BWT_ENCODED], BWT_BLOCK) for i, c in enumerate(enc)]
    dec += [c for c in cases if c.kind == "decode"]
    src = Guarded(BWT_ENCODED * len(dec), 0, np.concatenate([c.data for c in dec]), salt=3)
    dst = Guarded(BWT_BLOCK * len(dec), 0, salt=4)
    bwt_ctx.bwt_decode_device(src.view, BWT_ENCODED * len(dec), dst.view)
    bwt_ctx.sync_status()
    src.check(0, "decode src")
    dst.check(BWT_BLOCK * len(dec), "decode dst")
    back = dst.view.cpu().numpy()
    for i, c in enumerate(dec):
        check(stored, bad, c, (back[i * BWT_BLOCK: (i + 1) * BWT_BLOCK].tobytes(),))
    assert not bad, (len(bad), bad[:8])
    assert {crafted_cases.case_key(c) for c in enc + dec} == set(stored)


def test_every_stored_key_is_accounted_for():
    """Every key of the fixture is rebuilt by a test above or stands in the module's list of those that are not; made
    from the same selections the tests make, so a case that none of them takes shows up here."""
    rebuilt = set()
    for family in ENCODE_FAMILIES:
        rebuilt |= {crafted_cases.case_key(c) for c in encodes(family)}
    for family in DECODE_FAMILIES:
        rebuilt |= {crafted_cases.case_key(c) for c in of(family, "decode")}
    for family in ("truncations", "halving"):
        rebuilt |= {crafted_cases.case_key(c) for c in crafted_cases.cases(family) if c.kind == "stream_decode"}
    rebuilt |= {f"{k} chunked piece={p}" for k in list(rebuilt) if k.startswith("truncations/") and k.endswith("/stream_decode")
                for p in agreement_cases.TRUNCATION_PIECES}
    long = tuple(f"halving/{label}/" for label in crafted_cases.LONG)
    rebuilt |= {f"{k} chunked piece={resumable_cases.CHUNKED_PIECE}" for k in list(rebuilt)
                if k.startswith("halving/") and k.endswith("/stream_decode") and not k.startswith(long)}
    rebuilt |= set(agreement_cases.stored_crafted("bwt"))   # (test_block_sort asserts that it takes them all)
    stored = {k for family in crafted_cases.FAMILIES for k in agreement_cases.stored_crafted(family)}
    assert rebuilt <= stored
    rest = stored - rebuilt
    assert {k for k in rest if agreement_cases.device_key(k)} == LEFT_TO_OTHER_TESTS
    beyond = {k for k in rest if not agreement_cases.device_key(k)}
    carry = {k for k in beyond if k.startswith("carry/") and (" cap=" in k or k.endswith(" chunked piece=64"))}
    pieces = {k for k in beyond if k.startswith("halving/") and "/encode chunked piece=" in k}
    long_pieces = {f"halving/{label}/adaptive/stream_decode chunked piece={resumable_cases.CHUNKED_PIECE}" for label in crafted_cases.LONG}
    assert beyond == carry | pieces | long_pieces and len(pieces) == 5
