"""The premises of tests/static_cases.py, held to the oracle (and to the reference build where it is present): what the
GPU tests of the static coder's large totals and squeeze points rely on is true of their inputs."""
import numpy as np
import pytest

import static_cases as sc
from cpprcoder_amd import rcx

WRONG = {}  # table -> wrong_blocks(...), shared by the tests below


def wrong(name, ulps):
    if name not in WRONG:
        WRONG[name] = sc.wrong_blocks(name, ulps)
    return WRONG[name]


def header(stream):
    s = np.frombuffer(bytes(stream[:516]), np.uint8)
    return int(s[:4].view("<u4")[0]), s[4:516].view("<u2").astype(np.uint32)


def test_tables():
    t = sc.tables()
    assert [int(t[k].sum()) for k in ("near-flat", "near-flat/2", "near-flat/4", "flat")] == [16647552, 8323712, 4161792, 256 * 65535]
    assert all(v.shape == (256,) and int(v.max()) <= 65535 for v in t.values())
    assert int(t["random"].min()) >= 1 and int(t["random"].sum()) > 1 << 23
    assert int((t["half-zero"] == 0).sum()) == 128 and set(t["half-zero"]) == {0, 65535}
    cum = np.cumsum(t["half-zero"].astype(np.int64))
    assert int((np.diff(cum) == 0).sum()) == 128 - int(t["half-zero"][0] == 0)  # ties in cum: find()'s `<=`


def test_table_call_makes_streams_that_the_references_decode(oracle, reference):
    """rco_static_encode_table: the header holds the caller's counts and n, the oracle's decoder -- and the reference's own,
    where its build is present -- return the source; with the block's own histogram it is rco_static_encode."""
    for name, counts in sc.tables().items():
        blocks = sc.crafted_blocks(name)
        assert len(blocks) == sc.NBLOCKS
        for b, (data, stream) in enumerate(blocks):
            assert len(data) == sc.BLOCK
            n, hdr = header(stream)
            assert n == sc.BLOCK and np.array_equal(hdr, counts), (name, b)
            ok, out, size = oracle.static_decode(stream, sc.BLOCK)
            assert ok and size == sc.BLOCK and out == data.tobytes(), (name, b)
            if reference is not None and b % 8 == 0:
                ok, out, size = reference.static_decode(stream, sc.BLOCK)
                assert ok and size == sc.BLOCK and out == data.tobytes(), (name, b, "reference")
    for _, block, _ in sc.squeeze_ladder()[0][:20:3]:
        ok, want, _ = oracle.static_encode(block)
        assert ok and oracle.static_encode_table(sc.squeeze_points(block)[1], block).tobytes() == want
    with pytest.raises(RuntimeError):  # a byte whose count is 0
        oracle.static_encode_table(sc.tables()["half-zero"], np.arange(256, dtype=np.uint8))
    with pytest.raises(RuntimeError):  # a count that the header cannot hold
        oracle.static_encode_table(np.full(256, 65536, np.uint32), np.zeros(16, np.uint8))


def test_traces_are_the_decoder_state(oracle):
    """low and range in front of every symbol: replayed with true division they give the block back."""
    name = "random"
    counts = sc.tables()[name]
    total = int(counts.sum())
    data, stream, low, rng = next(iter(sc.crafted_blocks(name, trace=True)))
    assert int(rng[0]) == 0xFFFFFFFF and int(low[0]) == int.from_bytes(bytes(stream[517:521]), "big")
    t = rng // np.uint32(total)
    assert np.array_equal(sc.symbols_of(counts, low // t), data)
    assert sc.parent_decodes(counts, stream, 64, 0) == list(data[:64])


def test_what_the_arithmetic_before_the_fix_gets_wrong():
    """parent_estimate over the traces of the crafted blocks: the wrong targets (the failure that tests/test_lane_sim.py's
    target test reproduces when it is pointed at parent_estimate), and the blocks in which they name a wrong symbol.

    The condition that the crafted blocks were to meet -- a wrong symbol in at least 4 of 64 blocks with the exactly rounded
    reciprocal (near-flat, random), in at least 2 at half scale with +1 ulp -- cannot be met by any valid stream, whatever
    the seed or the number of blocks: top_slivers() shows that no stream reaches a target that those reciprocals get wrong
    (none of them for the exactly rounded one; 22 combinations of t and symbol at +1 ulp, which random blocks meet about
    once in 10^9 symbols).  What holds instead is asserted: every wrong target of those reciprocals is one too large; at -1
    ulp, where they are one too small, 14 near-flat blocks are decoded wrong; the flat and the half-zero table fail at +1
    ulp in 53 and 16 blocks; and static_cases.aimed_streams puts a low on the wrong targets of every reciprocal."""
    near = wrong("near-flat", (0, 1, -1))
    assert [near[u][1] for u in (0, 1, -1)] == [353951, 5110405, 664861]
    assert near[0][0] == [] and near[1][0] == [] and len(near[-1][0]) == 14
    rnd = wrong("random", (0, -1))
    assert rnd[0] == ([], 40446) and rnd[-1][1] == 34947 and len(rnd[-1][0]) == 3
    half = wrong("near-flat/2", (0, 1))
    assert half[0] == ([], 0) and half[1] == ([], 458191)
    assert len(wrong("flat", (1,))[1][0]) == 53 and len(wrong("half-zero", (1,))[1][0]) == 16
    for name, (ulp, blocks) in sc.MARKED.items():
        assert WRONG[name][ulp][0][:8] == blocks, name
    assert wrong("near-flat/4", (0, 1, -1)) == {u: ([], 0) for u in (0, 1, -1)}  # quotients below 2^22: exact


def test_no_valid_stream_reaches_a_target_that_is_one_too_large():
    assert sc.top_slivers("near-flat", 0) == [] and sc.top_slivers("random", 0) == []
    assert len(sc.top_slivers("near-flat/2", 1)) == 22


def test_aimed_streams(oracle):
    """Each puts the first or second low where parent_estimate names the neighbouring symbol, and the oracle decodes all
    of it."""
    have = {("near-flat", 0), ("near-flat", 1), ("near-flat", -1), ("random", 0), ("random", 1), ("random", -1),
            ("near-flat/2", 1), ("near-flat/2", -1), ("half-zero", 1), ("flat", 1)}
    for name, counts in sc.tables().items():
        for ulp in (0, 1, -1):
            streams = sc.aimed_streams(name, ulp)
            assert (len(streams) == 16) == ((name, ulp) in have) and len(streams) in (0, 16), (name, ulp)
            for s in streams:
                ok, out, size = oracle.static_decode(s, 4096)
                assert ok and size == 4096 and header(s) [0] == 4096
                assert sc.parent_decodes(counts, s, 2, ulp) != list(out[:2]), (name, ulp)


def test_squeeze_ladder(oracle):
    ladder, twice = sc.squeeze_ladder()
    assert len(ladder) == 64 and all(len(b) == sc.LADDER_BLOCK == 66560 for _, b, _ in ladder)
    names = [name for name, _, _ in ladder]
    for name, block, points in ladder + [("twice", twice, None)]:
        got, counts = sc.squeeze_points(block)
        ok, stream, _ = oracle.static_encode(block)
        assert ok and np.array_equal(header(stream)[1], counts & 0xFFFF), name  # the model of count() is the oracle's
        if points is not None:
            assert got == points, name
        for p in got:  # the squeeze is in front of the 65536th of the dominant byte (the ladder) or of a later 32768th
            assert block[p] == sc.DOMINANT
    assert len(twice) == 131072 and len(sc.squeeze_points(twice)[0]) == 2
    at = {name: points for name, _, points in ladder}
    assert at["p=65535"] == [65535] and at["p=66559"] == [66559] and at["p=65863"] == [65536 + 16 * 20 + 7]
    assert all(at[f"p={65536 + s}"] == [65536 + s] for s in range(16))
    assert at["p=65543 again"] == at["p=65543"]  # two blocks of the wave squeeze in the same piece, at the same place
    pieces = {p[0] // 16 for p in at.values() if p}
    assert len(pieces) >= 12  # and blocks that squeeze in different pieces
    by = {name: block for name, block, _ in ladder}
    piece = by["p=65541"][65536:65552]  # other symbols in front of and behind p, the dominant byte twice
    assert (piece[:5] != sc.DOMINANT).all() and piece[5] == sc.DOMINANT and (piece[6:] != sc.DOMINANT).any() and (piece[6:] == sc.DOMINANT).any()
    assert int(sc.squeeze_points(by["ends at 0xFFFE"])[1][sc.DOMINANT]) == 0xFFFE
    assert int(sc.squeeze_points(by["ends at 0xFFFF"])[1][sc.DOMINANT]) == 0xFFFF
    # `calm` (rcx_enc_static3_k): the largest count over the first EASY16 symbols + the symbols left < 0xFFFF
    def calm_sum(block):
        return int(np.bincount(block[: sc.EASY16], minlength=256).max()) + len(block) - sc.EASY16
    assert [calm_sum(by[k]) for k in ("calm 0xFFFE", "calm 0xFFFF", "calm 0x10000")] == [0xFFFE, 0xFFFF, 0x10000]
    assert at["calm 0xFFFF"] == [] and at["calm 0x10000"] == [66559]
    calm = [calm_sum(b) < 0xFFFF for _, b, _ in ladder]
    assert 10 <= sum(calm) <= 54  # one wave holds both kinds
    assert all(not at[n] for n, c in zip(names, calm) if c)  # a calm block cannot squeeze


def test_natural_inputs(oracle):
    block = sc.natural_block()
    assert len(block) == 16647552 <= rcx.MAX_BLOCK
    ok, stream, _ = oracle.static_encode(block)
    n, hdr = header(stream)
    assert ok and n == len(block) and np.array_equal(hdr, sc.NEAR_FLAT) and int(hdr.sum()) == 16647552  # no squeeze
    v = sc.natural_stream()
    assert rcx.MAX_BLOCK < len(v) == 1 << 24
    points, counts = sc.squeeze_points(v)
    ok, stream, _ = oracle.static_encode(v)
    n, hdr = header(stream)
    assert ok and n == len(v) and np.array_equal(hdr, counts)
    assert points == [65535] and int(hdr.sum()) == (1 << 24) - 32768 >= (1 << 24) - 40000
