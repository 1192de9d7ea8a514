"""CRC-32 per block and item on the GPU (include/rcx.h, "CRC-32 per block or per item") against zlib.crc32, and the
containers that verify on unpack.

The kernel reads an entry's aligned dwords row by row (64 lanes x 4 bytes), the up to 3 bytes in front of and behind them
one by one, and treats a lane's last dword apart: the shapes below cover every length 0 .. 1100 (every tail residue, no row
to four rows and a partial one) at every alignment, blocks from 16 bytes to RCX_MAX_BLOCK, and batches in which a wave's
entries differ by five orders of magnitude.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from cpprcoder_amd import container, rcx, workloads
from gpu_support import Guarded, ctx, oracle_decode_one  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise():
    """RCX_MAX_BLOCK random bytes (and 4 MiB more): every case below is a slice of them."""
    return np.random.RandomState(20250).randint(0, 256, rcx.MAX_BLOCK + (4 << 20) + 4096, dtype=np.uint8)


def zlib_items(data, offs):
    b = data.tobytes()
    return np.array([zlib.crc32(b[int(offs[i]): int(offs[i + 1])]) for i in range(len(offs) - 1)], np.uint32)


def zlib_blocks(data, block):
    b = data.tobytes()
    return np.array([zlib.crc32(b[at: at + block]) for at in range(0, len(b), block)], np.uint32)


def guarded(count):
    """Room for `count` results in a guarded buffer (gpu_support.Guarded) -> (the buffer, its middle as int32)."""
    whole = Guarded(4 * count, salt=7)
    return whole, whole.view.view(torch.int32)


def results(whole, count):
    """The first `count` results as uint32, after checking that nothing else of the buffer or around it changed."""
    whole.check(4 * count, "d_crc")
    return whole.view[: 4 * count].cpu().numpy().view(np.uint32).copy()


def items_on_gpu(ctx, d_src, offs):
    whole, mid = guarded(len(offs) - 1)
    ctx.crc32_items_device(d_src, offs, mid)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    return results(whole, len(offs) - 1)


def blocks_on_gpu(ctx, d_src, block):
    count = rcx.block_count(d_src.numel(), block)
    whole, mid = guarded(count)
    ctx.crc32_blocks_device(d_src, block, mid)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    return results(whole, count)


def as_i32(crcs):
    return torch.from_numpy(np.ascontiguousarray(crcs, np.uint32).view(np.int32).copy()).cuda()


# ---- vectors, lengths, alignments ------------------------------------------------------------------------------------
def test_known_vectors(ctx):
    parts = [b"123456789", b"", bytes(32), b"\xff" * 32]
    want = [0xCBF43926, 0, zlib.crc32(bytes(32)), zlib.crc32(b"\xff" * 32)]
    assert list(ctx.crc32_items(parts)) == want
    data = np.frombuffer(b"".join(parts), np.uint8)
    assert list(items_on_gpu(ctx, torch.from_numpy(data.copy()).cuda(), rcx.item_offsets([len(p) for p in parts]))) == want
    assert list(ctx.crc32_blocks(b"\xff" * 32, 32)) == [want[3]] and list(ctx.crc32_blocks(bytes(32), 16)) == [zlib.crc32(bytes(16))] * 2


def test_every_length_at_every_alignment(ctx, noise):
    lengths = np.arange(1101)
    offs = rcx.item_offsets(lengths)  # back to back: the running offsets take every value mod 16
    assert len({int(o) % 16 for o in offs[:-1]}) == 16
    total = int(offs[-1])
    data = noise[:total]
    want = zlib_items(data, offs)
    assert want[0] == 0
    room = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    d_data = torch.from_numpy(data).cuda()
    for shift in (0, 1, 3, 7, 8, 15):
        view = room[shift: shift + total]
        view.copy_(d_data)
        got = items_on_gpu(ctx, view, offs)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (shift, bad[:8], [hex(int(x)) for x in got[bad[:4]]])


def test_ragged_batch_with_one_long_item(ctx, noise):
    rs = np.random.RandomState(7)
    lengths = np.full(5001, 64)
    lengths[0] = 4 << 20
    lengths = lengths[rs.permutation(5001)]
    offs = rcx.item_offsets(lengths)
    data = noise[3: 3 + int(offs[-1])]
    want = zlib_items(data, offs)
    assert np.array_equal(items_on_gpu(ctx, torch.from_numpy(data).cuda(), offs), want)
    assert np.array_equal(ctx.crc32_items(data, lengths), want)  # the host-buffer call


def test_200000_items_of_64_bytes(ctx, noise):
    offs = rcx.item_offsets(np.full(200_000, 64))
    data = noise[1: 1 + int(offs[-1])]
    assert np.array_equal(items_on_gpu(ctx, torch.from_numpy(data).cuda(), offs), zlib_items(data, offs))


BLOCK_CASES = [(1, 16), (16, 16), (300_001, 16), (3 * 4096 - 7, 4096), (5 * 65536 + 1, 65536), ((3 << 20) + 5, 1 << 20),
               (rcx.MAX_BLOCK, rcx.MAX_BLOCK)]


@pytest.mark.parametrize("n,block", BLOCK_CASES)
def test_blocks(ctx, noise, n, block):
    data = noise[:n]
    want = zlib_blocks(data, block)
    assert len(want) == rcx.block_count(n, block)
    got = blocks_on_gpu(ctx, torch.from_numpy(data).cuda(), block)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (n, block, bad[:8])
    assert np.array_equal(ctx.crc32_blocks(data, block), got)  # the host-buffer call gives the same array


def test_blocks_in_a_buffer_of_any_alignment(ctx, noise):
    n, block = 7 * 4096 + 1234, 4096
    want = zlib_blocks(noise[:n], block)
    room = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    for shift in (1, 2, 3, 13):
        room[shift: shift + n].copy_(torch.from_numpy(noise[:n]).cuda())
        assert np.array_equal(blocks_on_gpu(ctx, room[shift: shift + n], block), want), shift


# ---- bounds and arguments ------------------------------------------------------------------------------------------------
def test_nothing_to_do_and_bad_arguments_write_nothing(ctx, noise):
    L, h = rcx.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    d_src = torch.from_numpy(noise[:4096]).cuda()
    whole, mid = guarded(16)
    offs = rcx.item_offsets([100, 200, 300])
    src, crc, o = d_src.data_ptr(), mid.data_ptr(), offs.ctypes.data
    # nothing to do
    assert L.rcx_crc32_blocks_device(h, src, 0, 4096, crc, stream) == rcx.OK
    assert L.rcx_crc32_verify_blocks_device(h, src, 0, 4096, crc, stream) == rcx.OK
    assert L.rcx_crc32_items_device(h, src, o, 0, crc, stream) == rcx.OK
    assert L.rcx_crc32_verify_items_device(h, src, o, 0, crc, stream) == rcx.OK
    assert L.rcx_crc32_blocks_device(h, None, 0, 4096, None, stream) == rcx.OK and L.rcx_crc32_items_device(h, None, None, 0, None, stream) == rcx.OK
    assert len(ctx.crc32_blocks(b"", 4096)) == 0 and len(ctx.crc32_items([])) == 0
    # RCX_E_ARG before anything is enqueued
    down = np.array([0, 100, 50, 300], np.uint64)
    long = np.array([0, rcx.MAX_BLOCK + 1], np.uint64)
    for st in (L.rcx_crc32_blocks_device(h, None, 4096, 4096, crc, stream), L.rcx_crc32_blocks_device(h, src, 4096, 4096, None, stream),
               L.rcx_crc32_verify_blocks_device(h, src, 4096, 4096, None, stream), L.rcx_crc32_verify_blocks_device(h, None, 4096, 4096, crc, stream),
               L.rcx_crc32_blocks_device(h, src, 4096, 15, crc, stream), L.rcx_crc32_blocks_device(h, src, 4096, rcx.MAX_BLOCK + 1, crc, stream),
               L.rcx_crc32_blocks_device(h, src, 4096, 0, crc, stream), L.rcx_crc32_verify_blocks_device(h, src, 4096, 8, crc, stream),
               L.rcx_crc32_blocks_device(None, src, 4096, 4096, crc, stream),
               L.rcx_crc32_items_device(h, None, o, 3, crc, stream), L.rcx_crc32_items_device(h, src, None, 3, crc, stream),
               L.rcx_crc32_items_device(h, src, o, 3, None, stream), L.rcx_crc32_verify_items_device(h, src, o, 3, None, stream),
               L.rcx_crc32_items_device(h, src, down.ctypes.data, 3, crc, stream), L.rcx_crc32_verify_items_device(h, src, down.ctypes.data, 3, crc, stream),
               L.rcx_crc32_items_device(h, src, long.ctypes.data, 1, crc, stream),
               L.rcx_crc32_blocks(h, None, 4096, 4096, crc), L.rcx_crc32_blocks(h, noise.ctypes.data, 4096, 15, crc),
               L.rcx_crc32_items(h, noise.ctypes.data, down.ctypes.data, 3, crc), L.rcx_crc32_items(h, None, o, 3, crc)):
        assert st == rcx.E_ARG
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # the latch is clean
    assert len(results(whole, 0)) == 0  # (not one of the 16 result words changed, nor anything around them)
    # and the context still works
    assert np.array_equal(items_on_gpu(ctx, d_src, offs), zlib_items(noise[:4096], offs))


def test_block_calls_need_no_reserve_and_take_any_stream(noise):
    fresh = rcx.Context(0)
    try:
        data = noise[: 9 * 4096 + 5]
        d_src = torch.from_numpy(data).cuda()
        whole, mid = guarded(10)
        expected = as_i32(zlib_blocks(data, 4096))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        fresh.crc32_blocks_device(d_src, 4096, mid, stream=side)
        fresh.verify_blocks_device(d_src, 4096, expected, stream=side)
        assert fresh.sync_status(stream=side, raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(results(whole, 10), zlib_blocks(data, 4096))
        assert fresh.scratch_bytes() == 0  # nothing was allocated for them
    finally:
        fresh.close()


# ---- verify ------------------------------------------------------------------------------------------------------------
def flip(d, at, bit=0x10):
    d[at] = int(d[at]) ^ bit


def test_verify_blocks(ctx, noise):
    block, n = 4096, 8 * 4096 + 777
    data = noise[5: 5 + n]
    d = torch.from_numpy(data).cuda()
    expected = as_i32(zlib_blocks(data, block))
    before = expected.clone()
    last = rcx.block_count(n, block) - 1
    ctx.verify_blocks_device(d, block, expected)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for k in (0, last // 2, last):
        first_byte, last_byte = k * block, min((k + 1) * block, n) - 1
        for at, bit in ((first_byte, 0x01), (last_byte, 0x80), (first_byte + 1, 0x08)):
            flip(d, at, bit)
            ctx.verify_blocks_device(d, block, expected)
            assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, k), (k, at)
            flip(d, at, bit)
    # two damaged blocks: the lower index; then a clean call on the same context
    flip(d, last * block + 3)
    flip(d, 3 * block + 100)
    ctx.verify_blocks_device(d, block, expected)
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, 3)
    flip(d, last * block + 3)
    flip(d, 3 * block + 100)
    ctx.verify_blocks_device(d, block, expected)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert torch.equal(expected, before) and np.array_equal(d.cpu().numpy(), data)  # verify wrote nothing


def test_verify_items(ctx, noise):
    lengths = np.array([300, 0, 1, 4096, 17, 0, 70_001, 64, 5, 1000])
    offs = rcx.item_offsets(lengths)
    data = noise[9: 9 + int(offs[-1])]
    d = torch.from_numpy(data).cuda()
    want = zlib_items(data, offs)
    expected = as_i32(want)
    ctx.verify_items_device(d, offs, expected)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for k in (0, 4, 6, 9):  # first, middle, the long one, the last
        for at, bit in ((int(offs[k]), 0x02), (int(offs[k + 1]) - 1, 0x40)):
            flip(d, at, bit)
            ctx.verify_items_device(d, offs, expected)
            assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, k), (k, at)
            flip(d, at, bit)
    flip(d, int(offs[9]) + 10)
    flip(d, int(offs[3]) + 10)
    ctx.verify_items_device(d, offs, expected)
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, 3)
    flip(d, int(offs[9]) + 10)
    flip(d, int(offs[3]) + 10)
    # an empty item is checked too: its CRC is 0
    wrong = want.copy()
    wrong[5] = 1
    ctx.verify_items_device(d, offs, as_i32(wrong))
    assert ctx.sync_status(raise_on_error=False) == (rcx.E_CORRUPT, 5)
    ctx.verify_items_device(d, offs, expected)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(d.cpu().numpy(), data)


# ---- the gap this closes: a damaged payload that still decodes ---------------------------------------------------------------
GAP_BLOCK = 4096


def silent_flips(oracle, streams, goods, want=3, limit=200):
    """Single-bit flips in a stream's payload that the oracle decodes completely, to other bytes than the original:
    -> [(stream index, byte in the stream, bit, what it decodes to)], scanning at most `limit` candidates.  (The oracle
    decodes one stream alone and reads no byte past it.)"""
    found, tried = [], 0
    for back in range(6, 6 + 64):  # towards the end of a stream a flip changes few symbols and little of what is read
        for b in range(len(streams)):
            if len(found) >= want or tried >= limit:
                return found, tried
            if any(f[0] == b for f in found) or back >= len(streams[b]) - 9:
                continue
            tried += 1
            s = streams[b].copy()
            at, bit = len(s) - back, 1 << (tried % 8)
            s[at] ^= bit
            ok, out = oracle_decode_one(oracle, s, len(goods[b]), 0, max(len(goods[b]), 16))
            if ok and not np.array_equal(out, goods[b]):
                found.append((b, at, bit, out))
    return found, tried


@pytest.fixture(scope="module")
def gap(oracle):
    """Zipf bytes, the adaptive coder, blocks of 4 KiB and a ragged last one; on the CPU: the oracle's streams and three
    flips that it decodes without complaint to wrong bytes."""
    n = 11 * GAP_BLOCK + 1500
    data = workloads.zipf(n, 77)
    slots, sizes = oracle.encode_blocks(data, GAP_BLOCK, threads=4)
    streams = [slots[b, : int(sizes[b])].copy() for b in range(len(sizes))]
    goods = [data[b * GAP_BLOCK: (b + 1) * GAP_BLOCK] for b in range(len(sizes))]
    flips, tried = silent_flips(oracle, streams, goods)
    return {"data": data, "streams": streams, "flips": flips, "tried": tried}


def damaged(blob, parsed, stream_index, at, bit):
    """`blob` with one bit of one stream's byte flipped."""
    out = bytearray(blob)
    out[len(blob) - len(parsed["payload"]) + int(parsed["offsets"][stream_index]) + at] ^= bit
    return bytes(out)


def test_silently_wrong_payloads_are_caught(gap, ctx):
    # on the CPU, before the GPU is touched: the oracle decodes every symbol of the damaged block, to other bytes
    assert len(gap["flips"]) >= 3, f"{len(gap['flips'])} silent flips among {gap['tried']} candidates"
    data = gap["data"]
    plain = container.pack(data, GAP_BLOCK, 0, ctx)
    checked = container.pack(data, GAP_BLOCK, 0, ctx, checksum=True)
    p1, p2 = container.parse(plain), container.parse(checked)
    assert plain[4] == 1 and checked[4] == 2 and p1["crcs"] is None
    assert np.array_equal(p1["payload"], np.concatenate(gap["streams"])) and np.array_equal(p2["payload"], p1["payload"])
    assert len(checked) == len(plain) + 4 * p1["nblocks"]
    for b, at, bit, wrong in gap["flips"]:
        expect = data.copy()
        expect[b * GAP_BLOCK: b * GAP_BLOCK + len(wrong)] = wrong
        # today's documented behaviour: wrong bytes, no complaint
        assert container.unpack(damaged(plain, p1, b, at, bit), ctx) == expect.tobytes() != data.tobytes()
        with pytest.raises(container.ChecksumError) as e:
            container.unpack(damaged(checked, p2, b, at, bit), ctx)
        assert e.value.index == b and e.value.kind == "block"
        assert container.unpack(damaged(checked, p2, b, at, bit), ctx, verify=False) == expect.tobytes()
    assert container.unpack(checked, ctx) == data.tobytes()
    # damage the decoder itself notices (a stream whose header disagrees with the layout) may surface as its RcxError
    with pytest.raises((container.ChecksumError, rcx.RcxError)):
        container.unpack(damaged(checked, p2, 4, 1, 0x01), ctx)
    assert container.unpack(checked, ctx) == data.tobytes()


def test_subsets_check_only_what_they_pick(gap, ctx, oracle):
    assert len(gap["flips"]) >= 3
    data = gap["data"]
    checked = container.pack(data, GAP_BLOCK, 0, ctx, checksum=True)
    p = container.parse(checked)
    b, at, bit, _ = gap["flips"][0]
    bad = damaged(checked, p, b, at, bit)
    lo, hi = (0, 1) if b >= 2 else (b + 1, b + 2)  # two blocks beside the damaged one
    assert container.unpack_range(bad, lo * GAP_BLOCK + 5, (hi + 1) * GAP_BLOCK - 5, ctx) == data[lo * GAP_BLOCK + 5: (hi + 1) * GAP_BLOCK - 5].tobytes()
    start, stop = max(b * GAP_BLOCK - 10, 0), min((b + 1) * GAP_BLOCK + 10, len(data))
    with pytest.raises(container.ChecksumError) as e:
        container.unpack_range(bad, start, stop, ctx)
    assert e.value.index == b  # the container's block, not the position among the picked ones
    assert container.unpack_range(bad, start, stop, ctx, verify=False) != data[start:stop].tobytes()
    assert container.unpack_range(checked, start, stop, ctx) == data[start:stop].tobytes()
    # items: the same with an item container
    lengths = [700, 0, 4096, 33, 2500, 0, 900, 16]
    cuts = rcx.item_offsets(lengths)
    items = [data[int(cuts[i]): int(cuts[i + 1])] for i in range(len(lengths))]
    blob = container.pack_items(items, 0, ctx, checksum=True)
    q = container.parse_items(blob)
    assert np.array_equal(q["crcs"], [zlib.crc32(x.tobytes()) for x in items])
    assert container.unpack_items(blob, ctx=ctx) == [x.tobytes() for x in items]
    plain = container.pack_items(items, 0, ctx)
    assert plain[4] == 1 and np.array_equal(container.parse_items(plain)["payload"], q["payload"])
    live = [i for i, n in enumerate(lengths) if n >= 500]
    streams = [np.array(q["payload"][int(q["offsets"][i]): int(q["offsets"][i + 1])]) for i in live]
    flips, tried = silent_flips(oracle, streams, [items[i] for i in live], want=1)
    assert flips, f"no silent flip among {tried} candidates"
    j, at, bit, wrong = flips[0]
    item = live[j]
    bad = damaged(blob, q, item, at, bit)
    rest = [i for i in range(len(lengths)) if i != item]
    assert container.unpack_items(bad, pick=rest[::-1], ctx=ctx) == [items[i].tobytes() for i in rest[::-1]]
    with pytest.raises(container.ChecksumError) as e:
        container.unpack_items(bad, pick=[rest[0], rest[1], item, rest[2]], ctx=ctx)
    assert e.value.index == item and e.value.kind == "item"
    with pytest.raises(container.ChecksumError):
        container.unpack_items(bad, ctx=ctx)
    assert container.unpack_items(bad, pick=[item], ctx=ctx, verify=False) == [wrong.tobytes()]
    assert container.unpack_items(damaged(plain, container.parse_items(plain), item, at, bit), pick=[item], ctx=ctx) == [wrong.tobytes()]


# ---- containers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text():
    return workloads.zipf(300_001, 5)


@pytest.mark.parametrize("coder", (0, 1, 2, 3))
def test_checked_containers_round_trip(ctx, oracle, text, coder):
    block = 4096
    blob = container.pack(text, block, coder, ctx, checksum=True)
    c = container.parse(blob)
    assert c["coder"] == coder and c["flags"] == container.FLAG_CRC32 and c["n"] == len(text)
    assert np.array_equal(c["crcs"], zlib_blocks(text, block))
    assert container.unpack(blob, ctx) == text.tobytes()
    # the block sort first: the checksums are of the coder's input, the sorted text
    blob = container.pack(text, block, coder, ctx, blksort=True, checksum=True)
    c = container.parse(blob)
    assert c["flags"] == container.FLAG_BLKSORT | container.FLAG_CRC32
    assert np.array_equal(c["crcs"], zlib_blocks(oracle.bwt_encode(text, threads=8), block))
    assert container.unpack(blob, ctx) == text.tobytes()
    plain = container.parse(container.pack(text, block, coder, ctx, blksort=True))
    assert plain["crcs"] is None and np.array_equal(plain["payload"], c["payload"]) and np.array_equal(plain["offsets"], c["offsets"])
    if coder == 0:
        assert container.unpack(container.pack(b"", block, coder, ctx, checksum=True), ctx) == b""
        assert container.unpack_items(container.pack_items([], coder, ctx, checksum=True), ctx=ctx) == []
        assert container.unpack_items(container.pack_items([b"", b""], coder, ctx, checksum=True), ctx=ctx) == [b"", b""]


# ---- the command line -------------------------------------------------------------------------------------------------------
def run_cli(*a):
    return subprocess.run([sys.executable, "-m", "cpprcoder_amd", *a], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=600)


def test_cli_round_trip_with_checksums(tmp_path, text):
    src = tmp_path / "in.bin"
    src.write_bytes(text.tobytes())
    r = run_cli("c", "--crc", "-b", "16384", str(src), str(tmp_path / "out.rcxb"))
    assert r.returncode == 0, r.stderr
    assert container.parse((tmp_path / "out.rcxb").read_bytes())["crcs"] is not None
    r = run_cli("d", str(tmp_path / "out.rcxb"), str(tmp_path / "back.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "back.bin").read_bytes() == src.read_bytes()
    r = run_cli("t", "--crc", "--coder", "rans8", str(src))
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr


def test_cli_refuses_to_write_a_damaged_file(tmp_path, gap, ctx):
    assert len(gap["flips"]) >= 3
    checked = container.pack(gap["data"], GAP_BLOCK, 0, ctx, checksum=True)
    b, at, bit, _ = gap["flips"][1]
    (tmp_path / "bad.rcxb").write_bytes(damaged(checked, container.parse(checked), b, at, bit))
    r = run_cli("d", str(tmp_path / "bad.rcxb"), str(tmp_path / "out.bin"))
    assert r.returncode == 1 and f"block {b}" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "out.bin").exists()
    r = run_cli("d", "--no-verify", str(tmp_path / "bad.rcxb"), str(tmp_path / "out.bin"))
    assert r.returncode == 0 and (tmp_path / "out.bin").read_bytes() != gap["data"].tobytes()
