"""Every device call on buffers and payloads past 4 GiB (tests/large_cases.py has the method: a tile of 8 MiB repeated 513
times on the device and 12 345 bytes more; period 256 begins at 2^31, period 512 at exactly 2^32).  Period 0 and the tail are held
to the CPU oracle or a numpy restatement, every later period to period 0 on the device; every comparison is exact.  The
decoders run on payloads tiled from the ORACLE's streams, which the encoders under test never produced.

A context per test, closed afterwards, and the allocator's cache emptied: the largest test (eight-state rANS) holds about 26
GiB on the device, none more than 32.  A test skips only if the device has less free memory than it needs, and prints both.
Only the host-buffer test holds arrays of 4 GiB in host memory.

Measured on an MI355X (pytest --durations=0, two runs: 39 tests in 47 s, none skipped, 287 GiB free), seconds per test:
    the largest blocks side by side   static 8.4 / 8.6 (64 lanes, 16 quads) and 3.7 / 3.8 (default), adaptive 4.5 and 3.6: one
                                      serial chain of 16.7 M symbols each way, as the host pipeline's comment says
    host-buffer calls                 3.9 (4.3 GB each way across the link, and the compares on the host)
    block coders                      0.16 - 0.31 a case, 0.7 - 1.3 the first of a coder (the oracle on the tile, once)
    item calls                        0.40 - 0.44;  planes and predictor 0.18 - 0.26 a case;  a damaged block 0.19
    block encoders read past 4 GiB    0.17 - 0.19;  filters, checksums and block sort read past 4 GiB 0.66
    block sort                        0.18 - 0.20;  stored items 0.2;  stored blocks 0.10;  typed items 0.06;  CRC and statistics 0.05
In each run three or four tests, other ones each time, took 1.7 - 4.9 s where their usual time is a fraction of a second (the
runtime giving back and taking tens of GiB of device memory between tests).  Nothing exceeded 10 s, so nothing is cut: both offsets,
both RCX_BWT_MATCH forms and the rerun in the default launch shape all run.
"""
import zlib

import numpy as np
import pytest

import large_cases as lc
import oracle_lib
import planes_cases
import predict_cases
import stats_cases
import typed_items_cases
from cpprcoder_amd import planes, predict, rcx, stats, stored, stored_items, typed_items, workloads
from gpu_support import CODERS, context, knobs, oracle_streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, T, K, TAIL, N, PER = lc.BLOCK, lc.T, lc.K, lc.TAIL, lc.N, lc.BLOCKS_PER_TILE
NBLOCKS = lc.NBLOCKS
GIB = 1 << 30
LIMIT_GIB = 32


@pytest.fixture
def fresh():
    """-> make(env=None): contexts of this test alone, closed behind it; then the allocator's cache is emptied."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    made = []

    def make(env=None):
        made.append(context(env))
        return made[-1]

    yield make
    for c in made:
        c.close()
    torch.cuda.empty_cache()


def need(gib):
    """Skip only if the device has less free memory than the test holds; the figures are printed either way."""
    assert gib <= LIMIT_GIB
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    print(f"needs {gib} GiB; free {free / GIB:.1f} GiB of {total / GIB:.1f} GiB")
    if free < gib * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free, the test holds {gib} GiB")


def i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def same(t, want):
    """A device tensor's bytes against a numpy array (small pieces only: period 0, the tail, picks)."""
    return np.array_equal(t.cpu().numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1))


# ---- block coders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("coder", CODERS)
def test_block_coders(fresh, oracle, coder, offset):
    """Encode N bytes: table and payload of period 0 and of the last block are the oracle's, periods 1 .. 512 equal period 0;
    decode the oracle's tiled payload into a guarded destination.  Again with every buffer at byte offset 3."""
    need(28)
    ctx = fresh()
    p0, o0, pt, ot = lc.oracle_blocks(oracle, coder)
    P = len(p0)
    src_whole, src = lc.on_device(lc.tile("coder"), offset)
    dst_whole, dst = lc.guarded(rcx.encode_bound(N, B, coder), offset)
    offs = torch.full((NBLOCKS + 1,), -1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(src, B, dst, offs, coder=coder)
    ctx.sync_status()
    total = int(offs[-1])
    assert total > 1 << 32
    assert total == lc.payload_bytes(oracle, coder)
    assert same(offs[: PER + 1], o0), "period 0's table differs from the oracle's"
    assert lc.periodic_table(offs, PER, K, "encode table") == P
    assert same(offs[K * PER:] - K * P, ot), "the last block's entries differ from the oracle's"
    assert same(dst[:P], p0), "period 0's streams differ from the oracle's"
    lc.periodic_equal(dst, P, K, "encode payload")
    assert same(dst[K * P: total], pt), "the last block's stream differs from the oracle's"
    assert lc.guards_intact(dst_whole, dst, written=total), "the encoder wrote outside [0, offsets[nblocks])"
    assert lc.guards_intact(src_whole, src)
    if coder in (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC):
        assert ctx.last_redo(NBLOCKS) == 0
    del dst, dst_whole, offs
    # the decoder, on streams the encoder above never produced
    comp_whole, comp, table = lc.tiled_streams(p0, o0, pt, ot, offset=offset)
    assert comp.numel() == total and int(table[-1]) == total
    out_whole, out = lc.guarded(N, offset, fill=0x5A)
    ctx.decode_blocks_device(comp, total, table, N, B, out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src), "round trip"
    assert lc.guards_intact(out_whole, out, fill=0x5A), "the decoder wrote outside its n bytes"
    assert lc.guards_intact(comp_whole, comp) and lc.guards_intact(src_whole, src)
    lc.periodic_equal(comp, P, K, "decode input")  # (not written)
    lc.periodic_equal(src, T, K, "source")
    if coder in (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC):
        assert ctx.last_redo(NBLOCKS) == 0


def test_a_damaged_block_past_4gib(fresh, oracle):
    """The declared length of one block of period 512 is flipped: RCX_E_CORRUPT and exactly that block, an index above 65536.
    With one of period 1 damaged as well: the lower index.  Every other block decodes."""
    need(16)
    ctx = fresh()
    p0, o0, pt, ot = lc.oracle_blocks(oracle, rcx.CODER_ADAPTIVE)
    _, src = lc.on_device(lc.tile("coder"))
    _, comp, table = lc.tiled_streams(p0, o0, pt, ot)
    assert int(table[-1]) > 1 << 32
    late, early = 512 * PER + 77, 1 * PER + 5
    assert late > 65536 and int(table[late]) > 1 << 32
    out_whole, out = lc.guarded(N, fill=0x5A)

    def run(damaged, want_bad):
        for b in damaged:
            comp[int(table[b])] ^= 1  # the lowest byte of the declared length: 65536 -> 65537
        out.fill_(0x5A)
        ctx.decode_blocks_device(comp, comp.numel(), table, N, B, out)
        st, bad = ctx.sync_status(raise_on_error=False)
        assert (st, bad) == (rcx.E_CORRUPT, want_bad)
        at = 0
        for b in sorted(damaged) + [NBLOCKS]:  # every other block decodes
            assert torch.equal(out[at * B: b * B], src[at * B: b * B]), f"blocks {at} .. {b} with {damaged} damaged"
            at = b + 1
        assert lc.guards_intact(out_whole, out, fill=0x5A)
        for b in damaged:
            comp[int(table[b])] ^= 1

    run([late], late)
    run([early, late], early)
    ctx.decode_blocks_device(comp, comp.numel(), table, N, B, out)  # and the payload is whole again
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK and torch.equal(out, src)


# ---- item calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_item_calls(fresh, oracle, coder):
    """The same buffer cut by a repeating pattern of lengths (0, 1, 16, 17, 4097, 65536, 65537, 200 000 and fill): the table and the
    streams are periodic and period 0 is oracle_streams; a shuffled pick of 500 items of periods 500 .. 512 with repeats into a small
    output; everything; RCX_E_CAPACITY with dst_cap just short."""
    need(30)
    ctx = fresh()
    x = lc.tile("coder")
    pattern = lc.item_pattern()
    tail = lc.cut_to(pattern, TAIL)
    lengths = lc.full_lengths(pattern, tail)
    per, nitems = len(pattern), len(lengths)
    soffs = rcx.item_offsets(lengths)
    assert int(soffs[-1]) == N
    want = oracle_streams(oracle, lc.items_of(x, pattern), coder)
    want_tail = oracle_streams(oracle, lc.items_of(x, tail), coder)
    sizes = np.array([0 if s is None else len(s) for s in want], np.int64)
    w0 = np.concatenate([s for s in want if s is not None])
    wt = np.concatenate([s for s in want_tail if s is not None])
    P = int(sizes.sum())
    _, src = lc.on_device(x)
    dst_whole, dst = lc.guarded(rcx.encode_items_bound(soffs, coder))
    table = torch.full((nitems + 1,), -1, dtype=torch.int64, device="cuda")
    ctx.encode_items_device(src, soffs, dst, table, coder=coder)
    ctx.sync_status()
    total = int(table[-1])
    assert total > 1 << 32
    assert total == K * P + len(wt)
    assert same(table[: per + 1], np.concatenate([[0], np.cumsum(sizes)])), "period 0's comp_offsets differ from the oracle's sizes"
    assert lc.periodic_table(table, per, K, "comp_offsets") == P
    assert same(table[K * per:] - K * P, np.concatenate([[0], np.cumsum([0 if s is None else len(s) for s in want_tail])]))
    assert same(dst[:P], w0), "period 0's streams differ from the oracle's"
    lc.periodic_equal(dst, P, K, "item streams")
    assert same(dst[K * P: total], wt), "the tail's streams differ from the oracle's"
    assert lc.guards_intact(dst_whole, dst, written=total)
    # a shuffled pick of 500 items, all from periods 500 .. 512 (the tail's items included), with repeats
    rs = np.random.RandomState(500 + coder)
    pick = rs.randint(500 * per, nitems, 380)
    pick = np.concatenate([pick, rs.choice(pick, 110), [nitems - 1, nitems - 1, 512 * per + int(np.argmax(pattern))] + list(range(nitems - 6, nitems - 1)),
                           [512 * per, 512 * per + 1]])
    rs.shuffle(pick)
    assert len(pick) == 500 and pick.min() >= 500 * per and len(set(pick.tolist())) < 500
    doffs = rcx.item_offsets(lengths[pick])
    small_whole, small = lc.guarded(int(doffs[-1]), 3, fill=0x5A)
    ctx.decode_items_device(dst, total, table, doffs, small, pick=pick, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = small.cpu().numpy()
    for k, i in enumerate(pick):
        at = int(soffs[i]) % T  # (an item never crosses a period's border)
        assert np.array_equal(got[int(doffs[k]): int(doffs[k + 1])], x[at: at + int(lengths[i])]), f"pick {k}: item {i}"
    assert lc.guards_intact(small_whole, small, fill=0x5A)
    del small, small_whole
    # everything
    out_whole, out = lc.guarded(N, fill=0x5A)
    ctx.decode_items_device(dst, total, table, soffs, out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src) and lc.guards_intact(out_whole, out, fill=0x5A)
    del out, out_whole
    # a destination just short: RCX_E_CAPACITY, index nitems, nothing written from dst + dst_cap on
    dst.fill_(0xA5)
    cap = total - 9
    ctx.encode_items_device(src, soffs, dst, table, coder=coder, dst_cap=cap)
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CAPACITY, nitems)
    assert lc.guards_intact(dst_whole, dst, written=cap), "written at or past dst + dst_cap"


# ---- byte planes and the predictor -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", [predict_cases.NONE, predict_cases.DELTA, predict_cases.ZIGZAG], ids=["planes", "delta", "zigzag"])
@pytest.mark.parametrize("width", planes_cases.WIDTHS)
def test_planes_and_predictor(fresh, width, pred):
    """rcx_planes_* (pred none) and rcx_predict_* (delta, zigzag), split and join on N bytes at offsets (0, 0) and (1, 3); the ragged
    last superblock and its N % width tail bytes lie past 2^32."""
    need(14)
    ctx = fresh()
    x = lc.tile("filter")
    if pred == predict_cases.NONE:
        want0, want_tail = planes_cases.split_numpy(x, width, B), planes_cases.split_numpy(lc.tail_of(x), width, B)
        split = lambda s, d: planes.split_device(ctx, s, width, B, d)  # noqa: E731
        join = lambda s, d: planes.join_device(ctx, s, width, B, d)  # noqa: E731
    else:
        want0, want_tail = predict_cases.split_numpy(x, width, B, pred), predict_cases.split_numpy(lc.tail_of(x), width, B, pred)
        split = lambda s, d: predict.split_device(ctx, s, width, B, pred, d)  # noqa: E731
        join = lambda s, d: predict.join_device(ctx, s, width, B, pred, d)  # noqa: E731
    assert (K * T) % (width * B) == 0 and K * T >= 1 << 32 and TAIL % width
    for a, b in ((0, 0), (1, 3)):
        src_whole, src = lc.on_device(x, a)
        dst_whole, dst = lc.guarded(N, b, fill=0x5A)
        split(src, dst)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert same(dst[:T], want0), "period 0 differs from the numpy restatement"
        lc.periodic_equal(dst, T, K, "split")
        assert same(dst[K * T:], want_tail), "the ragged last superblock differs from the numpy restatement"
        assert lc.guards_intact(dst_whole, dst, fill=0x5A) and lc.guards_intact(src_whole, src)
        lc.periodic_equal(src, T, K, "split source")  # (not written)
        back_whole, back = lc.guarded(N, a, fill=0x33)
        join(dst, back)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert torch.equal(back, src), "join(split(x)) is not x"
        assert lc.guards_intact(back_whole, back, fill=0x33) and lc.guards_intact(dst_whole, dst, fill=0x5A)
        del src, src_whole, dst, dst_whole, back, back_whole


def test_typed_items(fresh):
    """Items are the superblocks of all three widths with all three predictors in turn and runs of empty items, periodic in the tile;
    split, then join with both kernels (rows: no predictor; scan: delta and zigzag)."""
    need(14)
    ctx = fresh()
    x = lc.tile("filter")
    pattern = lc.typed_pattern()
    tail = lc.cut_typed(pattern, TAIL)
    lengths = lc.full_lengths(pattern[0], tail[0])
    widths, preds = (np.concatenate([np.tile(pattern[j], K), tail[j]]) for j in (1, 2))
    soffs = rcx.item_offsets(lengths)
    assert int(soffs[-1]) == N and set(preds.tolist()) == {0, 1, 2}
    want0 = typed_items_cases.split_expected({"lengths": pattern[0], "widths": pattern[1], "preds": pattern[2]}, x)
    want_tail = typed_items_cases.split_expected({"lengths": tail[0], "widths": tail[1], "preds": tail[2]}, lc.tail_of(x))
    assert not np.array_equal(want_tail, lc.tail_of(x))
    src_whole, src = lc.on_device(x, 1)
    dst_whole, dst = lc.guarded(N, 3, fill=0x5A)
    typed_items.split_device(ctx, src, soffs, widths, preds, dst)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert same(dst[:T], want0), "period 0 differs from the numpy restatement"
    lc.periodic_equal(dst, T, K, "typed split")
    assert same(dst[K * T:], want_tail), "the last item (past 2^32, cut short) differs from the numpy restatement"
    assert lc.guards_intact(dst_whole, dst, fill=0x5A) and lc.guards_intact(src_whole, src)
    back_whole, back = lc.guarded(N, 1, fill=0x33)
    typed_items.join_device(ctx, dst, soffs, widths, preds, back)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(back, src), "join(split(x)) is not x"
    assert lc.guards_intact(back_whole, back, fill=0x33) and lc.guards_intact(dst_whole, dst, fill=0x5A)


# ---- CRC-32 and statistics -----------------------------------------------------------------------------------------------------
def test_crc_and_statistics(fresh):
    """Block and item calls: period 0 and the tail against zlib.crc32, np.bincount and stats.cost_numpy, the rows periodic; verify
    with one wrong expectation in period 512 reports its index."""
    need(8)
    ctx = fresh()
    x = lc.tile("coder")
    _, src = lc.on_device(x, 3)
    pattern = lc.item_pattern()
    tail = lc.cut_to(pattern, TAIL)
    lengths = lc.full_lengths(pattern, tail)
    soffs = rcx.item_offsets(lengths)
    for what, per, count, parts0, parts_tail in (("blocks", PER, NBLOCKS, lc.items_of(x, [B] * PER), [lc.tail_of(x)]),
                                                 ("items", len(pattern), len(lengths), lc.items_of(x, pattern), lc.items_of(x, tail))):
        crc = torch.full((count + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        hist = torch.full((count * 256 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        cost = torch.full((count + 8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        if what == "blocks":
            ctx.crc32_blocks_device(src, B, crc)
            stats.blocks_device(ctx, src, B, hist, cost)
        else:
            ctx.crc32_items_device(src, soffs, crc)
            stats.items_device(ctx, src, soffs, hist, cost)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        for t in (crc, hist, cost):  # nothing written behind the tables
            assert same(t[-8:], np.full(8, 0x5A5A5A5A, {torch.int32: np.int32, torch.int64: np.int64}[t.dtype])), what
        want_crc = np.array([zlib.crc32(p.tobytes()) for p in parts0 + parts_tail], np.uint32)
        want_hist = np.stack([np.bincount(p, minlength=256) for p in parts0 + parts_tail]).astype(np.uint32)
        want_cost = stats.cost_numpy(want_hist)
        for name, t, want, row in (("crc", crc, want_crc, 1), ("hist", hist, want_hist, 256), ("cost", cost, want_cost, 1)):
            e = row * t.element_size()
            flat = t.view(torch.uint8)
            assert same(flat[: per * e], want[:per]), f"{what} {name}: period 0"
            lc.periodic_equal(flat, per * e, K, f"{what} {name}")
            assert same(flat[K * per * e: count * e], want[per:]), f"{what} {name}: the tail"
        # verify: right, then one wrong expectation in period 512
        wrong = 512 * per + per // 2 + 3
        assert wrong > 512 * per and (wrong > 65536 if what == "blocks" else lengths[wrong] > 0)
        verify = (lambda e: ctx.verify_blocks_device(src, B, e)) if what == "blocks" else (lambda e: ctx.verify_items_device(src, soffs, e))
        verify(crc)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK, what
        crc[wrong] ^= 1
        crc[count - 1] ^= 1
        verify(crc)
        assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, wrong), what


# ---- stored blocks and items ---------------------------------------------------------------------------------------------------
GAIN = 256  # 256 bytes of a 64 KiB block: a uniform block's stream expands, so it is stored; a special block's saves 700 and more and is kept


def test_stored_blocks(fresh, oracle):
    """rcx_stored_mix_device behind an encode: tables, flags and payload periodic, period 0 and the tail as stored.mix_numpy makes
    them of the oracle's streams; rcx_stored_decode_device of picks past 2^32, and of everything."""
    need(26)
    ctx = fresh()
    x, coder = lc.tile("coder"), rcx.CODER_ADAPTIVE
    p0, o0, pt, ot = lc.oracle_blocks(oracle, coder)
    want0, want_offs0, want_flags0 = stored.mix_numpy(x, B, p0, o0, GAIN)
    want_t, want_offs_t, want_flags_t = stored.mix_numpy(lc.tail_of(x), B, pt, ot, GAIN)
    kept = [b for b in range(PER) if not want_flags0[b]]
    assert kept == sorted(lc.SPECIAL_BLOCKS) and want_flags_t.tolist() == [1]  # most are stored, the special ones kept
    M = len(want0)
    _, src = lc.on_device(x)
    comp = torch.empty(rcx.encode_bound(N, B, coder), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(NBLOCKS + 1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(src, B, comp, offs, coder=coder)
    ctx.sync_status()
    assert int(offs[-1]) > 1 << 32
    mixed_whole, mixed = lc.guarded(N, 3)
    moffs = torch.full((NBLOCKS + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((NBLOCKS + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    stored.mix_device(ctx, src, B, comp, int(offs[-1]), offs, GAIN, mixed, moffs, flags)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    total = int(moffs[-1])
    assert total == K * M + len(want_t) and total > 1 << 32 and total < N
    assert same(moffs[: PER + 1], want_offs0) and lc.periodic_table(moffs, PER, K, "mixed table") == M
    assert same(moffs[K * PER:] - K * M, want_offs_t)
    assert same(flags[:PER], want_flags0) and same(flags[K * PER: NBLOCKS], want_flags_t) and same(flags[NBLOCKS:], np.full(8, 0x5A, np.uint8))
    lc.periodic_equal(flags, PER, K, "flags")
    assert same(mixed[:M], want0), "period 0 of the mix differs from stored.mix_numpy"
    lc.periodic_equal(mixed, M, K, "mixed payload")
    assert same(mixed[K * M: total], want_t) and lc.guards_intact(mixed_whole, mixed, written=total)
    del comp, offs
    # picks past 2^32 of the mixed payload: stored and kept blocks of period 512 and the short last one, shuffled, with repeats
    host_flags = np.concatenate([np.tile(want_flags0, K), want_flags_t])
    block_len = stored.block_lengths(N, B)
    first = 512 * PER + int(np.searchsorted(want_offs0.astype(np.int64), (1 << 32) - 512 * M))
    assert 512 * PER <= first < 512 * PER + kept[2] and 512 * M + int(want_offs0[first - 512 * PER]) >= 1 << 32
    rs = np.random.RandomState(11)
    pick = np.concatenate([rs.randint(first, NBLOCKS, 90), [512 * PER + kept[2], 512 * PER + kept[3], NBLOCKS - 1, NBLOCKS - 1]])
    rs.shuffle(pick)
    doffs = rcx.item_offsets(block_len[pick])
    small_whole, small = lc.guarded(int(doffs[-1]), 1, fill=0x5A)
    stored.decode_device(ctx, mixed, total, moffs, host_flags, doffs, small, pick=pick, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = small.cpu().numpy()
    for k, b in enumerate(pick):
        at = (int(b) * B) % T
        assert np.array_equal(got[int(doffs[k]): int(doffs[k + 1])], x[at: at + int(block_len[b])]), f"pick {k}: block {b}"
    assert lc.guards_intact(small_whole, small, fill=0x5A)
    del small, small_whole
    out_whole, out = lc.guarded(N, fill=0x5A)
    stored.decode_device(ctx, mixed, total, moffs, host_flags, rcx.item_offsets(block_len), out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src) and lc.guards_intact(out_whole, out, fill=0x5A)


def test_stored_items(fresh, oracle):
    """rcx_stored_mix_items_device behind the item encode, on the item pattern: tables, flags and payload periodic, period 0 and the
    tail as stored_items.mix_items_numpy makes them of the oracle's streams; then everything back through rcx_stored_decode_device."""
    need(26)
    ctx = fresh()
    x, coder = lc.tile("coder"), rcx.CODER_ADAPTIVE
    pattern = lc.item_pattern()
    tail = lc.cut_to(pattern, TAIL)
    lengths = lc.full_lengths(pattern, tail)
    per, nitems = len(pattern), len(lengths)
    soffs = rcx.item_offsets(lengths)
    want, want_mix = [], []
    for part, cut in ((x, pattern), (lc.tail_of(x), tail)):
        streams = oracle_streams(oracle, lc.items_of(part, cut), coder)
        sizes = np.array([0 if s is None else len(s) for s in streams], np.int64)
        payload = np.concatenate([s for s in streams if s is not None])
        want.append((payload, np.concatenate([[0], np.cumsum(sizes)])))
        want_mix.append(stored_items.mix_items_numpy(part, rcx.item_offsets(cut), payload, want[-1][1], GAIN))
    (want0, want_offs0, want_flags0), (want_t, want_offs_t, want_flags_t) = want_mix
    assert 0 < int(want_flags0.sum()) < int((pattern > 0).sum())  # both kinds: stored and kept
    M = len(want0)
    _, src = lc.on_device(x)
    comp = torch.empty(rcx.encode_items_bound(soffs, coder), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nitems + 1, dtype=torch.int64, device="cuda")
    ctx.encode_items_device(src, soffs, comp, offs, coder=coder)
    ctx.sync_status()
    assert int(offs[-1]) > 1 << 32
    mixed_whole, mixed = lc.guarded(N, 3)
    moffs = torch.full((nitems + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((nitems + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    stored_items.mix_items_device(ctx, src, soffs, comp, int(offs[-1]), offs, GAIN, mixed, moffs, flags)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    total = int(moffs[-1])
    assert total == K * M + len(want_t) and total > 1 << 32
    assert same(moffs[: per + 1], want_offs0) and lc.periodic_table(moffs, per, K, "mixed table") == M
    assert same(moffs[K * per:] - K * M, want_offs_t)
    assert same(flags[:per], want_flags0) and same(flags[K * per: nitems], want_flags_t) and same(flags[nitems:], np.full(8, 0x5A, np.uint8))
    lc.periodic_equal(flags, per, K, "flags")
    assert same(mixed[:M], want0), "period 0 of the mix differs from stored_items.mix_items_numpy"
    lc.periodic_equal(mixed, M, K, "mixed payload")
    assert same(mixed[K * M: total], want_t) and lc.guards_intact(mixed_whole, mixed, written=total)
    del comp, offs
    out_whole, out = lc.guarded(N, fill=0x5A)
    stored.decode_device(ctx, mixed, total, moffs, flags[:nitems].cpu().numpy(), soffs, out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src) and lc.guards_intact(out_whole, out, fill=0x5A)


# ---- block sort ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", ["ballot", "atomic"])
def test_block_sort(fresh, oracle, match):
    """bwt_encode_device / bwt_decode_device on N bytes, in both forms of the counting pass's rank (RCX_BWT_MATCH, as
    gpu_support.bwt_ctx sets it): the rows of enc.view(-1, 32770) are periodic, period 0 is oracle.bwt_encode of the tile, the
    tail is copied, and the round trip returns the source."""
    need(16)
    x = lc.tile("coder")
    rows, unit = T // rcx.BWT_BLOCK, rcx.BWT_ENCODED
    size = rcx.bwt_encode_bound(N)
    assert size == K * rows * unit + TAIL and rcx.bwt_decoded_size(size) == N
    want0 = oracle.bwt_encode(x, threads=8)
    assert len(want0) == rows * unit
    with knobs({"RCX_BWT_MATCH": match}):  # (read at the context's first block-sort call)
        ctx = fresh()
        _, src = lc.on_device(x, 1)
        enc_whole, enc = lc.guarded(size, 3, fill=0x5A)
        ctx.bwt_encode_device(src, enc)
        ctx.sync_status()
        assert same(enc[: rows * unit], want0), "period 0 differs from the oracle's block sort"
        lc.periodic_equal(enc, rows * unit, K, "block sort")
        assert enc[: K * rows * unit].view(-1, unit).shape[0] == K * rows
        assert same(enc[K * rows * unit:], lc.tail_of(x)), "the tail is not copied"
        assert lc.guards_intact(enc_whole, enc, fill=0x5A)
        back_whole, back = lc.guarded(N, 1, fill=0x33)
        ctx.bwt_decode_device(enc, size, back)
        ctx.sync_status()
        assert torch.equal(back, src), "round trip"
        assert lc.guards_intact(back_whole, back, fill=0x33) and lc.guards_intact(enc_whole, enc, fill=0x5A)


# ---- sources past 2^32 are read where they lie ---------------------------------------------------------------------------------
# Period 512 begins at exactly 2^32 and repeats period 0, so a SOURCE position that wrapped there would read equal bytes, and no test
# above would notice.  Here period 512 and the tail hold the other tile (large_cases.on_device, `last`): their results must be those of
# that tile, from the oracle and the numpy restatements, and periods 1 .. 511 still equal period 0.
@pytest.mark.parametrize("coder", CODERS)
def test_block_encoders_read_past_4gib(fresh, oracle, coder):
    need(28)
    ctx = fresh()
    p0, o0, _, _ = lc.oracle_blocks(oracle, coder)
    pl, ol, pt, ot = lc.oracle_blocks(oracle, coder, "filter")
    P, L = len(p0), len(pl)
    assert not np.array_equal(p0[:4096], pl[:4096])
    _, src = lc.on_device(lc.tile("coder"), 3, last=lc.tile("filter"))
    dst_whole, dst = lc.guarded(rcx.encode_bound(N, B, coder))
    offs = torch.full((NBLOCKS + 1,), -1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(src, B, dst, offs, coder=coder)
    ctx.sync_status()
    total, base = int(offs[-1]), 512 * P
    assert total > 1 << 32 and base > 1 << 32
    assert total == base + L + len(pt)
    assert same(offs[: PER + 1], o0) and lc.periodic_table(offs, PER, 512, "encode table") == P
    assert same(offs[512 * PER: K * PER + 1] - base, ol), "period 512's table is not the oracle's of the bytes that lie there"
    assert same(offs[K * PER:] - base - L, ot)
    assert same(dst[:P], p0)
    lc.periodic_equal(dst, P, 512, "encode payload")
    assert same(dst[base: base + L], pl), "period 512's streams are not the oracle's of the bytes that lie there"
    assert same(dst[base + L: total], pt), "the last block's stream"
    assert lc.guards_intact(dst_whole, dst, written=total)
    out_whole, out = lc.guarded(N, fill=0x5A)
    ctx.decode_blocks_device(dst, total, offs, N, B, out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src) and lc.guards_intact(out_whole, out, fill=0x5A)


def test_filters_checksums_and_block_sort_read_past_4gib(fresh, oracle):
    """The same for the calls that read a source of N bytes by position alone: plane filter and predictor (every width once), typed
    items, CRC-32 and statistics per block, the item encoder, the block sort."""
    need(14)
    ctx = fresh()
    x, y = lc.tile("filter"), lc.tile("coder")  # periods 0 .. 511 hold x, period 512 and the tail y
    at = 512 * T
    assert at == 1 << 32
    _, src = lc.on_device(x, 1, last=y)
    dst_whole, dst = lc.guarded(N, 3, fill=0x5A)
    for width, pred in ((2, predict_cases.NONE), (4, predict_cases.DELTA), (8, predict_cases.ZIGZAG)):
        dst.fill_(0x5A)
        if pred == predict_cases.NONE:
            planes.split_device(ctx, src, width, B, dst)
            want = [planes_cases.split_numpy(part, width, B) for part in (x, y, lc.tail_of(y))]
        else:
            predict.split_device(ctx, src, width, B, pred, dst)
            want = [predict_cases.split_numpy(part, width, B, pred) for part in (x, y, lc.tail_of(y))]
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
        assert same(dst[:T], want[0])
        lc.periodic_equal(dst, T, 512, f"split {width} {pred}")
        assert same(dst[at: at + T], want[1]), f"width {width}, predictor {pred}: period 512 is not the transform of the bytes that lie there"
        assert same(dst[at + T:], want[2]), f"width {width}, predictor {pred}: the ragged last superblock"
        assert lc.guards_intact(dst_whole, dst, fill=0x5A)
    # typed items
    pattern = lc.typed_pattern()
    tail = lc.cut_typed(pattern, TAIL)
    lengths = lc.full_lengths(pattern[0], tail[0])
    widths, preds = (np.concatenate([np.tile(pattern[j], K), tail[j]]) for j in (1, 2))
    case, case_tail = ({"lengths": c[0], "widths": c[1], "preds": c[2]} for c in (pattern, tail))
    dst.fill_(0x5A)
    typed_items.split_device(ctx, src, rcx.item_offsets(lengths), widths, preds, dst)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    lc.periodic_equal(dst, T, 512, "typed split")
    assert same(dst[:T], typed_items_cases.split_expected(case, x)) and same(dst[at: at + T], typed_items_cases.split_expected(case, y))
    assert same(dst[at + T:], typed_items_cases.split_expected(case_tail, lc.tail_of(y)))
    del dst, dst_whole
    # CRC-32 and statistics per block
    crc = torch.zeros(NBLOCKS, dtype=torch.int32, device="cuda")
    hist = torch.zeros(NBLOCKS * 256, dtype=torch.int32, device="cuda")
    cost = torch.zeros(NBLOCKS, dtype=torch.int64, device="cuda")
    ctx.crc32_blocks_device(src, B, crc)
    stats.blocks_device(ctx, src, B, hist, cost)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    parts = lc.items_of(y, [B] * PER) + [lc.tail_of(y)]
    want_hist = stats_cases.hist_blocks(np.concatenate([y, lc.tail_of(y)]), B)
    assert same(crc[512 * PER:], np.array([zlib.crc32(p.tobytes()) for p in parts], np.uint32)), "CRC-32 of period 512 and the tail"
    assert same(hist[512 * PER * 256:], want_hist) and same(cost[512 * PER:], stats.cost_numpy(want_hist)), "counts and costs of period 512 and the tail"
    assert same(crc[:PER], np.array([zlib.crc32(p.tobytes()) for p in lc.items_of(x, [B] * PER)], np.uint32))
    lc.periodic_equal(crc.view(torch.uint8), 4 * PER, 512, "crc")
    lc.periodic_equal(cost.view(torch.uint8), 8 * PER, 512, "cost")
    del crc, hist, cost
    # the item encoder (adaptive): the streams of period 512 and the tail are those of y's items
    item_pattern = lc.item_pattern()
    item_tail = lc.cut_to(item_pattern, TAIL)
    per = len(item_pattern)
    soffs = rcx.item_offsets(lc.full_lengths(item_pattern, item_tail))
    streams = [[s for s in oracle_streams(oracle, lc.items_of(part, cut), 0) if s is not None]
               for part, cut in ((x, item_pattern), (y, item_pattern), (lc.tail_of(y), item_tail))]
    w0, w512, wt = (np.concatenate(s) for s in streams)
    comp = torch.full((rcx.encode_items_bound(soffs, 0),), 0x5A, dtype=torch.uint8, device="cuda")
    table = torch.zeros(len(soffs), dtype=torch.int64, device="cuda")
    ctx.encode_items_device(src, soffs, comp, table)
    ctx.sync_status()
    base = 512 * len(w0)
    assert lc.periodic_table(table, per, 512, "comp_offsets") == len(w0) and int(table[512 * per]) == base
    assert int(table[-1]) == base + len(w512) + len(wt) and int(table[K * per]) == base + len(w512)
    lc.periodic_equal(comp, len(w0), 512, "item streams")
    assert same(comp[: len(w0)], w0) and same(comp[base: base + len(w512)], w512) and same(comp[base + len(w512): int(table[-1])], wt)
    del comp, table
    # the block sort
    rows, unit = T // rcx.BWT_BLOCK, rcx.BWT_ENCODED
    enc = torch.full((rcx.bwt_encode_bound(N),), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.bwt_encode_device(src, enc)
    ctx.sync_status()
    lc.periodic_equal(enc, rows * unit, 512, "block sort")
    assert same(enc[: rows * unit], oracle.bwt_encode(x, threads=8))
    assert same(enc[512 * rows * unit: K * rows * unit], oracle.bwt_encode(y, threads=8)), "period 512 is not the block sort of the bytes that lie there"
    assert same(enc[K * rows * unit:], lc.tail_of(y))


# ---- host-buffer calls -----------------------------------------------------------------------------------------------------------
def test_host_buffer_calls(fresh, oracle):
    """encode_blocks_into / decode_blocks_into with the adaptive coder on a numpy source of N bytes, destinations with a 64-byte
    canary: the table is periodic and the device call's, the payload period-equal on the host (and period 0 the oracle's), the
    canaries intact.  The only test with arrays of 4 GiB in host memory."""
    need(30)
    ctx = fresh()
    x, coder = lc.tile("coder"), rcx.CODER_ADAPTIVE
    p0, o0, pt, ot = lc.oracle_blocks(oracle, coder)
    P = len(p0)
    host = np.empty(N, np.uint8)  # np.tile(x, K) and the tail, without a second copy
    host[: K * T].reshape(K, T)[:] = x
    host[K * T:] = lc.tail_of(x)
    bound = rcx.encode_bound(N, B, coder)
    dst = np.full(bound + 64, 0xA5, np.uint8)
    table = np.full(NBLOCKS + 1 + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    size = ctx.encode_blocks_into(host, B, dst[:bound], table[: NBLOCKS + 1], coder=coder)
    assert size > 1 << 32 and size == int(table[NBLOCKS]) == lc.payload_bytes(oracle, coder)
    assert bool((table[NBLOCKS + 1:] == 0xA5A5A5A5A5A5A5A5).all()) and bool((dst[bound:] == 0xA5).all()), "canary"
    assert bool((dst[size: size + (1 << 20)] == 0xA5).all()), "written past the payload"
    offsets = table[: NBLOCKS + 1].astype(np.int64)
    assert lc.periodic_table(offsets, PER, K, "host table") == P
    assert np.array_equal(offsets[: PER + 1], o0.astype(np.int64)) and np.array_equal(offsets[K * PER:] - K * P, ot.astype(np.int64))
    assert np.array_equal(dst[:P], p0) and np.array_equal(dst[K * P: size], pt)
    lc.periodic_equal(dst, P, K, "host payload")
    # the device call's table
    _, src = lc.on_device(x)
    d_dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(NBLOCKS + 1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(src, B, d_dst, d_offs, coder=coder)
    ctx.sync_status()
    assert same(d_offs, offsets), "the host call's table is not the device call's"
    del src, d_dst, d_offs
    torch.cuda.empty_cache()
    out = np.full(N + 64, 0x5A, np.uint8)
    got = ctx.decode_blocks_into(dst[:size], size, table[: NBLOCKS + 1], B, out[:N], coder=coder)
    assert got == N and bool((out[N:] == 0x5A).all()), "canary"
    lc.periodic_equal(out, T, K, "host round trip")
    assert np.array_equal(out[:T], x) and np.array_equal(out[K * T: N], lc.tail_of(x))


# ---- entry limits ------------------------------------------------------------------------------------------------------------
def test_entry_limits(fresh):
    """2^31 blocks (block 16) and 2^31 items are RCX_E_ARG before anything is enqueued: the small buffers handed over are unchanged."""
    need(1)
    ctx = fresh()
    L, h, s = rcx.lib(), ctx._h, torch.cuda.current_stream().cuda_stream
    n = 16 << 31
    assert rcx.block_count(n, 16) == 0x80000000 and rcx.block_count(n - 16, 16) == 0x7FFFFFFF
    bufs = [lc.guarded(4096, fill=f) for f in (0x11, 0x22, 0x33)]
    (_, a), (_, b), (_, c) = bufs
    assert L.rcx_encode_blocks_device(h, 0, a.data_ptr(), n, 16, b.data_ptr(), 1 << 40, c.data_ptr(), s) == rcx.E_ARG
    assert L.rcx_decode_blocks_device(h, 0, a.data_ptr(), 4096, c.data_ptr(), 0x80000000, 16, n, b.data_ptr(), s) == rcx.E_ARG
    table = np.zeros(64, np.uint64)
    assert L.rcx_encode_items_device(h, 0, a.data_ptr(), table.ctypes.data, 0x80000000, b.data_ptr(), 4096, c.data_ptr(), s) == rcx.E_ARG
    assert L.rcx_decode_items_device(h, 0, a.data_ptr(), 4096, c.data_ptr(), 0x80000000, None, 1, table.ctypes.data, b.data_ptr(), s) == rcx.E_ARG
    assert L.rcx_decode_items_device(h, 0, a.data_ptr(), 4096, c.data_ptr(), 8, None, 0x80000000, table.ctypes.data, b.data_ptr(), s) == rcx.E_ARG
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for (whole, view), f in zip(bufs, (0x11, 0x22, 0x33)):
        assert lc.all_bytes(whole, f)


# ---- 64 largest blocks in one workgroup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [{"RCX_ENC_LANES": "64", "RCX_DEC_QUADS": "16"}, {}], ids=["64 lanes, 16 quads", "default"])
@pytest.mark.parametrize("coder", [rcx.CODER_ADAPTIVE, rcx.CODER_STATIC], ids=["adaptive", "static"])
def test_the_largest_blocks_side_by_side(fresh, oracle, golden, coder, shape):
    """65 copies of the golden zipf(NO_HALVING,4) block (RCX_MAX_BLOCK bytes each, 1.02 GiB), 64 of them to a workgroup where the
    shape says so: a lane's slot offset (lane * slot) is at its largest.  Stream 0 has the golden's size and fnv1a64 (the static
    coder: the oracle's stream), streams 1 .. 64 equal stream 0, decode returns the source."""
    need(8)
    ctx = fresh(shape)
    copies, block = 65, rcx.MAX_BLOCK
    data = workloads.zipf(block, 4)
    g = golden["long"]["adaptive"]["zipf(NO_HALVING,4)"]
    assert oracle_lib.sha(data) == g["input_sha256"] and g["n"] == block
    if coder == rcx.CODER_ADAPTIVE:
        size, fnv = g["size"], g["fnv1a64"]
    else:
        slots, sizes = oracle.encode_blocks(data, block, coder=coder)
        size, fnv = int(sizes[0]), "%016x" % oracle_lib.fnv1a64(slots[0, : int(sizes[0])])
    n = copies * block
    src = torch.from_numpy(data).cuda().repeat(copies)
    dst_whole, dst = lc.guarded(rcx.encode_bound(n, block, coder))
    offs = torch.full((copies + 1,), -1, dtype=torch.int64, device="cuda")
    ctx.encode_blocks_device(src, block, dst, offs, coder=coder)
    ctx.sync_status()
    assert lc.periodic_table(offs, 1, copies, "table") == size
    assert "%016x" % oracle_lib.fnv1a64(dst[:size].cpu().numpy()) == fnv, "stream 0 is not the reference's"
    lc.periodic_equal(dst, size, copies, "streams", step=8)
    assert lc.guards_intact(dst_whole, dst, written=copies * size)
    assert ctx.last_redo(copies) == 0
    out_whole, out = lc.guarded(n, fill=0x5A)
    ctx.decode_blocks_device(dst, copies * size, offs, n, block, out, coder=coder)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(out, src) and lc.guards_intact(out_whole, out, fill=0x5A)
    assert ctx.last_redo(copies) == 0
