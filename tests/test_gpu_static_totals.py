"""The static range coder (csrc/rcx_static.hpp, four kernels) at totals up to 2^24 - 256 and at the places where count()'s
16-bit squeeze (cpprcoder.h:549-555) can fall; inputs and their premises: tests/static_cases.py, tests/test_static_cases_cpu.py.

* Crafted blocks: streams the oracle made with a given table (totals 4.2 M ... 16.8 M in blocks of 262144 symbols), decoded
  by the four-lane kernel, by the one-lane kernel (RCX_LANES_PER_BLOCK=1), and as single streams into a sink of n and of
  n - 1 bytes (the one-lane STREAM path); with a flipped payload byte (the one-lane kernel as the pass behind the four-lane
  one); and aimed streams, whose low sits on a target that the one-lane decoder's arithmetic got wrong before
  rcx_static_target -- with the exactly rounded reciprocal no valid stream reaches one.
* The two natural inputs with a total near 2^24: a block of 16 647 552 bytes through both encoders and both decoders, a
  stream of 2^24 bytes through the single-stream calls.
* The squeeze ladder through the three-wave encoder (alone in a workgroup and 64 to a workgroup), the one-wave encoder
  and the plain path.
"""
import numpy as np
import pytest

import agreement_cases
import crafted_cases
import static_cases as sc
from cpprcoder_amd import rcx
from gpu_support import assert_same_blocks, check_blocks, context, ctx, gpu_decode, gpu_encode, oracle_decode_one  # noqa: F401

pytestmark = pytest.mark.gpu

STATIC = rcx.CODER_STATIC
TABLES = list(sc.tables())


@pytest.fixture(scope="module")
def one_lane():
    c = context({"RCX_LANES_PER_BLOCK": "1"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def encoders(ctx):
    """The default context (so few blocks: one to a workgroup of the three-wave encoder), the one-wave encoder, and the
    three-wave encoder with 64 blocks to a workgroup whatever the device's compute unit count."""
    made = {"one wave": context({"RCX_ENC_VARIANT": "0"}), "64 lanes": context({"RCX_ENC_LANES": "64"})}
    yield {"default": ctx, **made}
    for c in made.values():
        c.close()


def joined(streams):
    offsets = np.zeros(len(streams) + 1, np.uint64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    return np.concatenate(streams), offsets


# ---- crafted blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_crafted_blocks_by_both_decoders(ctx, one_lane, name):
    blocks = sc.crafted_blocks(name)
    data = np.concatenate([d for d, _ in blocks])
    payload, offsets = joined([s for _, s in blocks])
    back, st, _ = gpu_decode(ctx, payload, offsets, len(data), sc.BLOCK, coder=STATIC)
    assert st == 0 and np.array_equal(back, data), "four lanes a block"
    assert ctx.last_redo(len(blocks)) == 0  # (no valid stream is left to the pass behind)
    back, st, _ = gpu_decode(one_lane, payload, offsets, len(data), sc.BLOCK, coder=STATIC, comp_offset=3)
    bad = [b for b in range(len(blocks)) if not np.array_equal(back[b * sc.BLOCK: (b + 1) * sc.BLOCK], blocks[b][0])]
    assert st == 0 and not bad, f"one lane a block: blocks {bad}"


@pytest.mark.parametrize("name", TABLES)
def test_crafted_single_streams(ctx, oracle, name):
    """rcx_stream_decode into a sink of n bytes (the four-lane kernel) and of n - 1 (rcx_dec_static_k<STREAM>): the blocks
    in which the arithmetic before rcx_static_target names a wrong symbol with some reciprocal within 1 ulp
    (static_cases.MARKED: eight of them at the most), and four others."""
    blocks = sc.crafted_blocks(name)
    marked = sc.MARKED.get(name, (0, []))[1]
    for b in marked + [b for b in (0, 21, 42, 63) if b not in marked]:
        data, stream = blocks[b]
        for cap in (sc.BLOCK, sc.BLOCK - 1):
            ok, want, _ = oracle.static_decode(stream, cap)
            st, _, out = ctx.stream_decode(stream, cap, coder=STATIC)
            assert ok and st == rcx.OK and len(out) == cap, (name, b, cap, st, len(out))
            assert out == want == data.tobytes()[:cap], (name, b, cap)


def expected_of(oracle, streams, n):
    """-> (status, first bad stream or None, per stream the oracle's bytes or None where it fails)."""
    want = []
    for s in streams:
        ok, out = oracle_decode_one(oracle, s, n, STATIC, n)
        want.append(out if ok else None)
    bad = [i for i, w in enumerate(want) if w is None]
    return (rcx.E_CORRUPT if bad else rcx.OK), (bad[0] if bad else None), want


def check_against(oracle, c, streams, n, label):
    payload, offsets = joined(streams)
    want_st, want_first, want = expected_of(oracle, streams, n)
    back, st, first = gpu_decode(c, payload, offsets, n * len(streams), n, coder=STATIC)
    assert st == want_st and (want_first is None or first == want_first), (label, st, first, want_st, want_first)
    for i, w in enumerate(want):
        assert w is None or np.array_equal(back[i * n: (i + 1) * n], w), (label, i)


@pytest.mark.parametrize("name", sc.LARGE)
def test_crafted_blocks_with_a_flipped_byte(ctx, one_lane, oracle, name):
    """Two of eight crafted streams with one payload byte flipped (and padded, so that the reference decodes on to the end,
    where the table lets it): status, first failing block and bytes are the oracle's, from the four-lane kernel with the
    one-lane pass behind it and from the one-lane kernel alone."""
    rs = np.random.RandomState(31 + TABLES.index(name))
    blocks = sc.crafted_blocks(name)[8:16]
    streams = [s for _, s in blocks]
    for b in (2, 5):
        s = np.concatenate([streams[b], rs.randint(0, 256, 3 * sc.BLOCK).astype(np.uint8)])
        s[int(rs.randint(600, len(streams[b]) // 2))] ^= 0x10
        streams[b] = s
    _, _, want = expected_of(oracle, streams, sc.BLOCK)
    assert all(want[b] is None or not np.array_equal(want[b], blocks[b][0]) for b in (2, 5))  # the flips matter
    check_against(oracle, ctx, streams, sc.BLOCK, (name, "default"))
    check_against(oracle, one_lane, streams, sc.BLOCK, (name, "one lane"))


@pytest.mark.parametrize("name", ["near-flat", "near-flat/2", "random", "half-zero", "flat"])
def test_aimed_streams(ctx, one_lane, oracle, name):
    """Streams whose first or second low lies where the one-lane decoder's target was wrong before rcx_static_target, for
    the exactly rounded reciprocal and for one 1 ulp either side (static_cases.aimed_streams): both decoders, and the
    single-stream call into a sink one byte short, return what the oracle returns."""
    n = 4096
    streams = [s for ulp in (0, 1, -1) for s in sc.aimed_streams(name, ulp, n=n)]
    assert len(streams) >= 16
    check_against(oracle, ctx, streams, n, (name, "default"))
    check_against(oracle, one_lane, streams, n, (name, "one lane"))
    for i, s in enumerate(streams):
        ok, want, _ = oracle.static_decode(s, n - 1)
        st, _, out = ctx.stream_decode(s, n - 1, coder=STATIC)
        assert ok and st == rcx.OK and out == want, (name, i)


# ---- the natural inputs ----------------------------------------------------------------------------------------------------
def test_natural_block_of_total_16647552(encoders, one_lane, oracle):
    """Byte i exactly 65535 - (37 i mod 1024) times: the block's own count() gives the near-flat table.  Both encoders make
    the oracle's stream, both decoders return the block.  (As large as tests/test_gpu_parity.py's
    test_block_of_the_largest_size: a total of 2^24 needs 2^24 symbols.)"""
    data = sc.natural_block()
    ok, want, size = oracle.static_encode(data)
    assert ok
    for name in ("default", "one wave"):
        payload, offsets, _ = gpu_encode(encoders[name], data, len(data), coder=STATIC)
        assert int(offsets[-1]) == size and payload.tobytes() == want, name
    for name, c in (("four lanes", encoders["default"]), ("one lane", one_lane)):
        back, st, _ = gpu_decode(c, payload, offsets, len(data), len(data), coder=STATIC)
        assert st == 0 and np.array_equal(back, data), name
    assert encoders["default"].last_redo(1) == 0


def test_natural_stream_of_two_to_the_24(ctx, oracle):
    """2^24 bytes, one early squeeze, total 2^24 - 32768: past RCX_MAX_BLOCK, so rcx_enc_static_k and rcx_dec_static_k code
    it as a single stream.  The kernel's stream is the oracle's, and it has the digest the real reference build's stream has
    (tests/golden/reference_crafted.json: the one static encode that tests/test_gpu_reference_digests.py leaves to this test,
    which codes the 2^24 symbols on one lane anyway)."""
    v = sc.natural_stream()
    ok, want, size = oracle.static_encode(v)
    st, _, comp = ctx.stream_encode(v, coder=STATIC)
    assert ok and st == rcx.OK and len(comp) == size and comp == want
    assert agreement_cases.digest((comp,)) == agreement_cases.stored_crafted("static")[crafted_cases.NATURAL_STREAM + "/static/encode"]
    st, _, back = ctx.stream_decode(comp, len(v), coder=STATIC)
    assert st == rcx.OK and back == v.tobytes()


# ---- the squeeze ladder ----------------------------------------------------------------------------------------------------
def encode_and_back(c, oracle, data, block, label, src_offset=0):
    nblocks = rcx.block_count(len(data), block)
    slots, sizes = oracle.encode_blocks(data, block, coder=STATIC, threads=8)
    payload, offsets, _ = gpu_encode(c, data, block, src_offset=src_offset, coder=STATIC)
    if label[0] != "one wave":  # (the one-wave encoder is itself the pass behind the three-wave one: it marks nothing)
        assert c.last_redo(nblocks) == 0, label
    assert_same_blocks(payload, offsets, slots, sizes, label)
    back, st, _ = gpu_decode(c, payload, offsets, len(data), block, coder=STATIC)
    assert st == 0 and np.array_equal(back, data) and c.last_redo(nblocks) == 0, label


@pytest.mark.parametrize("shape", ["default", "one wave", "64 lanes"])
def test_squeeze_ladder(encoders, oracle, shape):
    """64 blocks of 66560 bytes (static_cases.squeeze_ladder): alone in their workgroups each block takes its own side of
    `calm`; 64 to a workgroup the wave is not calm and wave 0 counts every block in order, the squeezes falling in different
    16-byte pieces, twice in the same one, and not at all.  Then 64 calm blocks, the one at 0xFFFE among them (64 to a
    workgroup: the only wave whose three waves all count past symbol 65535), and the block with two squeezes."""
    ladder, twice = sc.squeeze_ladder()
    encode_and_back(encoders[shape], oracle, sc.ladder_bytes(), sc.LADDER_BLOCK, (shape, "ladder"))
    calm = [b for name, b, _ in ladder if name.startswith("calm") and name not in ("calm 0xFFFF", "calm 0x10000")]
    assert len(calm) >= 16
    encode_and_back(encoders[shape], oracle, np.concatenate([calm[i % len(calm)] for i in range(64)]), sc.LADDER_BLOCK, (shape, "calm wave"))
    encode_and_back(encoders[shape], oracle, twice, len(twice), (shape, "two squeezes"))


def test_squeeze_ladder_on_the_plain_path(encoders, oracle):
    """The source one byte behind a 16-byte border and a short last block: `full` is false, every symbol is counted one by
    one (rcx_static_count_checked<false>), in both encoders."""
    data = np.concatenate([sc.ladder_bytes(), sc.squeeze_ladder()[0][3][1][:1000]])
    for shape in ("default", "one wave", "64 lanes"):
        encode_and_back(encoders[shape], oracle, data, sc.LADDER_BLOCK, (shape, "plain"), src_offset=1)
