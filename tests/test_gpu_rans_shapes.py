"""The rANS kernels (csrc/rcx_rans.hpp) on the paths a property of the data picks, or of the neighbouring blocks in the
wave: every stream byte for byte against the oracle -- the header with the model's table is part of the stream -- and
decoded back.  The inputs are tests/rans_cases.py's; tests/test_rans_cases_cpu.py holds them to what is claimed here.

* The model (rcx_rans_model): the steal loop's victim in every lane's range, on a tie between two lanes, worn down to 1 and
  replaced within a block, steals in both directions, 196 / 240 of them from one symbol (victim_cases, singletons); as
  single blocks, side by side in one call with a different model in every octet of a wave, and through the stream calls.
* The encoders' output rings (RCX_RANS8_DRAIN, rcx_rans1w_pipeline, rcx_enc_rans1_k's acc / nacc): 255 symbols of range 1 in
  a row at every phase of the rounds and chunks (dense_rare), one symbol of frequency 4096 / 16384 (one_symbol).
* Wave-wide minima and maxima over blocks of different lengths (common, by_eights, fast_groups, max_groups, even, out8;
  maxlen, nchunks): the item calls with chosen lengths side by side, aligned and not, every third item a run of rare
  symbols; the oracle's streams are decoded, not the encoder's.  The eight-state kernels always seat eight blocks a wave
  and rcx_enc_rans1w_k 64 a workgroup; the one-state DECODER seats 1 ... 16 by the call's entry count -- one with as few
  entries as these calls have, every quad of a wave then on the same block -- so it also decodes under RCX_DEC_QUADS = 16
  and 4, where a wave holds 16 or 4 different entries of the work order (rans_cases.quad_waves).
* FULL on and off at nchunks 1 ... 4: 128 whole blocks of 16 ... 64 bytes, aligned and not, and with a 5-byte block more.
* The one-wave one-state encoder (RCX_RANS1_WAVES=1, RCX_RANS1_LANES = 1 ... 16), which nothing else runs.

Measured on an MI355X, per test (the oracle's share included): every case as one block 0.8 s (one-state) and 0.1 s
(eight-state); the stream calls 0.5 and 0.1 s; the dense runs' decodes 0.25 and 0.05 s; the cases side by side 0.11 - 0.17 s
a call of 4.4 MiB; the small whole blocks 0.14 s; the one-wave encoder 0.10 s; the item tests 0.07 - 0.10 s (the one-state
ones in three decoder shapes); the 41 tests together 8.5 s, the start of the process included.
"""
import numpy as np
import pytest

import rans_cases
from cpprcoder_amd import rcx, workloads
from gpu_support import assert_same_blocks, assert_same_items, check_blocks, context, ctx, decode_items, encode_items, gpu_decode, gpu_encode  # noqa: F401
from gpu_support import oracle_streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RANS = (rcx.CODER_RANS, rcx.CODER_RANS8)
IDS = ["rans", "rans8"]


@pytest.fixture(scope="module")
def blocks():
    return rans_cases.block_cases()


# ---- model and ring inputs as blocks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_every_case_as_one_block(ctx, oracle, blocks, coder):
    """A block call of one block, of exactly the case's length (16 at the least, the smallest block size)."""
    for name, block in blocks.items():
        check_blocks(ctx, oracle, block, max(len(block), 16), coder=coder, label=(name, coder))


@pytest.fixture(scope="module")
def padded(oracle, blocks):
    """The cases in one call, a block of 131072 bytes each -> {filler: (data, {coder: the oracle's (slots, sizes)})}, made once."""
    out = {}
    for filler in ("seeded", "dominant"):
        data = rans_cases.padded_call(blocks, filler)
        out[filler] = (data, {coder: oracle.encode_blocks(data, rans_cases.PADDED_BLOCK, coder=coder, threads=16) for coder in RANS})
    return out


@pytest.mark.parametrize("filler", ["seeded", "dominant"])
@pytest.mark.parametrize("src_offset", [0, 8, 5])
@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_the_cases_side_by_side_in_one_call(ctx, padded, coder, src_offset, filler):
    """Eight blocks to a wave of the model kernel and of the eight-state coders, each with a model of its own; filled up
    with its most frequent byte a case keeps its losers: a steal loop of over 200 rounds next to one of none."""
    data, want = padded[filler]
    block = rans_cases.PADDED_BLOCK
    payload, offsets, _ = gpu_encode(ctx, data, block, src_offset=src_offset, coder=coder)
    assert_same_blocks(payload, offsets, *want[coder], label=(coder, src_offset, filler))
    back, st, _ = gpu_decode(ctx, payload, offsets, len(data), block, dst_offset=src_offset, coder=coder)
    assert st == 0 and np.array_equal(back, data), (coder, src_offset, filler)


@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_dense_runs_decode_at_every_alignment(ctx, oracle, coder):
    """The oracle's stream of every dense_rare block, to a destination and from a stream on a 16-byte border, 8 and 2 behind
    one (words still even-aligned), and at odd addresses."""
    for head in rans_cases.DENSE_RARE_HEADS:
        data = rans_cases.dense_rare(head)
        payload, offsets = oracle.compact(*oracle.encode_blocks(data, len(data), coder=coder))
        for dst_offset, comp_offset in ((0, 0), (8, 2), (1, 1)):
            back, st, _ = gpu_decode(ctx, payload, offsets, len(data), len(data), dst_offset=dst_offset, comp_offset=comp_offset, coder=coder)
            assert st == 0 and np.array_equal(back, data), (head, dst_offset, comp_offset)


# ---- wave mixes through the item calls -------------------------------------------------------------------------------------
OFFSETS = ((0, 0, 0, 0), (8, 8, 8, 8), (1, 1, 1, 1), (0, 8, 1, 8), (8, 1, 8, 1))   # source, destination, compressed, output


def mixed_items(lengths, seed):
    """Slices of the Zipf and Canterbury workloads, every third item a run of rare symbols among zeros."""
    pools = (workloads.zipf(8192, seed), workloads.by_name("canterbury", 8192, seed))
    items = []
    for k, n in enumerate(lengths):
        if k % 3 == 2:
            items.append(rans_cases.rare_item(n, seed + k))
        else:
            at = (131 * k) % (8192 - n + 1)
            items.append(pools[k % 3][at: at + n].copy())
    return items


def compact(streams):
    offs = np.zeros(len(streams) + 1, np.uint64)
    np.cumsum([len(s) for s in streams], out=offs[1:])
    return np.concatenate(streams), offs


@pytest.fixture(scope="module")
def decoders(ctx):
    """coder -> {shape: context} to decode with.  The one-state decoder (rcx_dec_rans1_quad_k) seats decode_quads() blocks a
    wave: 1 for the few entries of these calls, all 16 quads of a wave then on one block and every wave-wide maximum that
    block's own.  Forced to 16 and to 4 (read when a context is made), a wave holds that many entries of different
    lengths.  The eight-state decoder's shape is fixed."""
    forced = {f"{q} quads": context({"RCX_DEC_QUADS": str(q)}) for q in (16, 4)}
    yield {rcx.CODER_RANS: {"default": ctx, **forced}, rcx.CODER_RANS8: {"default": ctx}}
    for c in forced.values():
        c.close()


def both_ways(ctx, decoders, items, want, coder, pick=None, label=None):
    """At every OFFSETS: the GPU's streams of `items` are `want`; the GPU decodes `want` (the picked ones) to the items, in
    every launch shape of `decoders`."""
    want_payload, want_offs = compact(want)
    picked = items if pick is None else [items[int(k)] for k in pick]
    for src_offset, dst_offset, comp_offset, out_offset in OFFSETS:
        at = (label, coder, src_offset, dst_offset, comp_offset, out_offset)
        payload, offs = encode_items(ctx, items, coder, src_offset=src_offset, dst_offset=dst_offset)
        assert_same_items(payload, offs, want, at)
        for shape, c in decoders[coder].items():
            back, st, _ = decode_items(c, want_payload, want_offs, [len(x) for x in picked], coder, pick=pick, comp_offset=comp_offset, dst_offset=out_offset)
            assert st == rcx.OK, (at, shape)
            for k, x in enumerate(picked):
                assert np.array_equal(back[k], x), (at, shape, k, len(x))


@pytest.mark.parametrize("name", list(rans_cases.LENGTH_SETS))
@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_chosen_lengths_side_by_side(ctx, decoders, oracle, coder, name):
    items = mixed_items(rans_cases.LENGTH_SETS[name], 40 + len(name))
    both_ways(ctx, decoders, items, oracle_streams(oracle, items, coder), coder, label=name)


@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_mixed_lengths_in_reversed_order_with_a_shuffled_pick(ctx, decoders, oracle, coder):
    """The caller's order is not the work order, and the pick is neither."""
    items = mixed_items(rans_cases.WAVE_MIXED, 77)[::-1]
    pick = np.random.RandomState(78).permutation(len(items))
    assert not np.array_equal(pick, np.arange(len(items)))
    both_ways(ctx, decoders, items, oracle_streams(oracle, items, coder), coder, pick=pick, label="mixed, reversed")


# ---- FULL on and off at small chunk counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [16, 32, 48, 64])
@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_whole_small_blocks_with_full_on_and_off(ctx, decoders, oracle, coder, block):
    """128 whole blocks (two workgroups of rcx_enc_rans1w_k, every lane with a block) of 1 ... 4 chunks: from a 16-byte
    border FULL holds everywhere -- nchunks 1 ... 4 cross the look-ahead's `nchunks > 1` and `c >= 2` --, 4 bytes behind one
    it holds nowhere, and with a block of 5 bytes more it fails in that block's workgroup alone.  The one-state decoder's
    FULL likewise, in waves of one block (the default for 128 blocks), of 16 and of 4: the 5-byte block then has a wave to
    itself, or idle quads beside it.  The eight-state decoder has 2, 4, 6 and 8 groups here: fast_groups is 0 but for the last."""
    for tail in (0, 5):
        data = workloads.by_name("canterbury", 128 * block + tail, 900 + block + tail)
        slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=8)
        assert len(sizes) == 128 + (tail != 0)
        for src_offset in (0, 4):
            payload, offsets, _ = gpu_encode(ctx, data, block, src_offset=src_offset, coder=coder)
            assert_same_blocks(payload, offsets, slots, sizes, (coder, block, tail, src_offset))
        for shape, c in decoders[coder].items():
            for dst_offset in (0, 4):
                back, st, _ = gpu_decode(c, payload, offsets, len(data), block, dst_offset=dst_offset, coder=coder)
                assert st == 0 and np.array_equal(back, data), (coder, block, tail, shape, dst_offset)


# ---- the one-wave one-state encoder ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_wave_references(oracle):
    """(data, block, the oracle's slots, sizes) for rcx_enc_rans1_k, made once: two dense runs and the singletons as one
    block each, and 70 blocks of 4096 bytes, the last one ragged."""
    cases = [(d, len(d)) for d in (rans_cases.dense_rare(0), rans_cases.dense_rare(15), rans_cases.singletons())]
    cases.append((workloads.by_name("canterbury", 69 * 4096 + 1370, 950), 4096))
    return [(data, block, *oracle.encode_blocks(data, block, coder=rcx.CODER_RANS, threads=8)) for data, block in cases]


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16])
def test_the_one_wave_encoder(ctx, one_wave_references, monkeypatch, lanes):
    """RCX_RANS1_WAVES=1 selects rcx_enc_rans1_k, RCX_RANS1_LANES its blocks per wave; from a 16-byte border it takes 16
    symbols at a time behind the ragged end, 5 bytes behind one every symbol alone.  That the variables select that kernel
    is taken from the code (rcx_launch.hpp encode_launches() reads them with getenv at every launch); the library reports
    no kernel names and both encoders owe the same bytes, so the test cannot tell which one ran."""
    monkeypatch.setenv("RCX_RANS1_WAVES", "1")
    monkeypatch.setenv("RCX_RANS1_LANES", str(lanes))
    for data, block, slots, sizes in one_wave_references:
        for src_offset in (0, 5):
            payload, offsets, _ = gpu_encode(ctx, data, block, src_offset=src_offset, coder=rcx.CODER_RANS)
            assert_same_blocks(payload, offsets, slots, sizes, (lanes, len(data), block, src_offset))
        back, st, _ = gpu_decode(ctx, payload, offsets, len(data), block, coder=rcx.CODER_RANS)
        assert st == 0 and np.array_equal(back, data), (lanes, len(data), block)


# ---- the stream calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", RANS, ids=IDS)
def test_the_stream_calls(ctx, oracle, coder):
    """rcx_stream_encode runs the octet kernel rcx_enc_rans_k<false> for the one-state format, which no block call does."""
    cases = {f"victims, {k}": v for k, v in rans_cases.victim_cases().items()}
    cases.update({"singletons": rans_cases.singletons(), "dense_rare(7)": rans_cases.dense_rare(7), "one_symbol(9)": rans_cases.one_symbol(9)})
    for name, data in cases.items():
        st, _, comp = ctx.stream_encode(data, coder=coder)
        assert st == 0 and comp == oracle.rans_encode(data, simd=(coder == rcx.CODER_RANS8)), (name, coder)
        st, _, back = ctx.stream_decode(comp, max(len(data), 16), coder=coder)
        assert st == 0 and back == data.tobytes(), (name, coder)
