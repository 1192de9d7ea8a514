"""The byte-plane filter on the GPU (include/rcx_planes.h; csrc/rcx_planes.hpp) against its numpy restatement
(tests/planes_cases.py), and the typed container on top of it against the CPU oracle.

A lane's unit is 16 elements, a workgroup's step RCX_PLANES_U4 / width rows of 256 units; what is not a whole unit goes byte
by byte.  The shapes: n around one element, one unit and one superblock, with a ragged fourth superblock, for blocks of
16, 48 and 100 bytes (less than a step; 100: planes off 16-byte borders) and 4096, source and destination at every offset of
(0, 1, 3, 8, 15), every buffer guarded; and 8 MiB + 5 bytes at 64 KiB blocks, where the fixed grid loops.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import planes_cases as pc
from cpprcoder_amd import container, planes, rcx
from gpu_support import CODERS, Guarded, ctx, oracle_decode_one, run_filter  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20251).randint(0, 256, (8 << 20) + 64, dtype=np.uint8)


@pytest.fixture(scope="module")
def bf16():
    return pc.randn_bytes("bf16")[0]


def run(ctx, join, x, width, block, src_offset=0, dst_offset=0):
    """gpu_support.run_filter of one plane call."""
    fn = planes.join_device if join else planes.split_device
    return run_filter(ctx, lambda src, dst: fn(ctx, src, width, block, dst), f"{'join' if join else 'split'} w={width} B={block}", x, src_offset, dst_offset)


# ---- the kernel against numpy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", pc.WIDTHS)
def test_split_and_join_against_numpy(ctx, noise, width):
    cases = [c for c in pc.kernel_cases() if c[0] == width]
    assert len(cases) == 48
    for k, (_, block, n, so, do) in enumerate(cases):
        x = noise[k: k + n]
        y = pc.split_numpy(x, width, block)
        got = run(ctx, False, x, width, block, so, do)
        bad = np.flatnonzero(got != y)
        assert len(bad) == 0, ("split", width, block, n, so, do, bad[:8])
        back = run(ctx, True, y, width, block, do, so)
        bad = np.flatnonzero(back != x)
        assert len(bad) == 0, ("join", width, block, n, do, so, bad[:8])


@pytest.mark.parametrize("width", pc.WIDTHS)
def test_eight_mebibytes_and_five_bytes(ctx, noise, width):
    n, block = (8 << 20) + 5, 65536
    x = noise[3: 3 + n]
    y = pc.split_numpy(x, width, block)
    assert np.array_equal(run(ctx, False, x, width, block), y)
    assert np.array_equal(run(ctx, True, y, width, block), x)
    # in a whole superblock, coder block s * w + p is plane p
    s, p = 5, width - 1
    assert np.array_equal(y[(s * width + p) * block: (s * width + p + 1) * block], x[s * width * block + p: (s + 1) * width * block: width])


def test_host_buffer_calls(ctx, noise):
    for width, block, n in ((2, 4096, 3 * 8192 + 5), (4, 100, 1234), (8, 65536, (1 << 20) + 3), (4, 16, 0)):
        x = noise[:n]
        y = planes.split(ctx, x, width, block)
        assert y == pc.split_numpy(x, width, block).tobytes(), (width, block, n)
        assert planes.join(ctx, y, width, block) == x.tobytes(), (width, block, n)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(ctx, noise):
    L, h = planes.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    src = Guarded(n, 0, noise[:n], salt=1)
    dst = Guarded(n, 0, salt=2)
    room = Guarded(3 * n, 0, noise[: 3 * n], salt=3)  # one allocation for the overlapping and the adjacent ranges
    s, d, r = src.view.data_ptr(), dst.view.data_ptr(), room.view.data_ptr()
    host_out = np.full(n, 0xA5, np.uint8)
    for fn in (L.rcx_planes_split_device, L.rcx_planes_join_device):
        # nothing to do
        assert fn(h, s, 0, 2, 4096, d, stream) == rcx.OK and fn(h, None, 0, 8, 16, None, stream) == rcx.OK
        for st in (fn(h, s, n, 0, 4096, d, stream), fn(h, s, n, 1, 4096, d, stream), fn(h, s, n, 3, 4096, d, stream), fn(h, s, n, 16, 4096, d, stream),
                   fn(h, s, n, 6, 4096, d, stream),                                                     # the width
                   fn(h, s, n, 4, 15, d, stream), fn(h, s, n, 4, 0, d, stream), fn(h, s, n, 4, rcx.MAX_BLOCK + 1, d, stream),  # the block
                   fn(h, s, 0, 3, 4096, d, stream), fn(h, s, 0, 4, 15, d, stream),                      # ... also with nothing to do
                   fn(h, None, n, 4, 4096, d, stream), fn(h, s, n, 4, 4096, None, stream),              # null pointers
                   fn(None, s, n, 4, 4096, d, stream),
                   fn(h, r, n, 4, 4096, r, stream), fn(h, r, n, 4, 4096, r + 1, stream), fn(h, r + 1, n, 4, 4096, r, stream),  # overlaps
                   fn(h, r, n, 4, 4096, r + n - 1, stream), fn(h, r + n - 1, n, 4, 4096, r, stream)):
            assert st == rcx.E_ARG
    for fn in (L.rcx_planes_split, L.rcx_planes_join):
        for st in (fn(h, noise.ctypes.data, n, 5, 4096, host_out.ctypes.data), fn(h, noise.ctypes.data, n, 4, 8, host_out.ctypes.data),
                   fn(h, None, n, 4, 4096, host_out.ctypes.data), fn(h, noise.ctypes.data, n, 4, 4096, None),
                   fn(h, noise.ctypes.data, n, 4, 4096, noise.ctypes.data + 100)):
            assert st == rcx.E_ARG
        assert fn(h, None, 0, 4, 4096, None) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for g, what in ((src, "src"), (dst, "dst"), (room, "room")):
        g.check(0, what)  # not a byte changed anywhere
    assert bool((host_out == 0xA5).all())
    # ranges that touch are apart: the second third of the allocation from its first, and the first from the second
    y = pc.split_numpy(noise[:n], 4, 4096)
    assert L.rcx_planes_split_device(h, r, n, 4, 4096, r + n, stream) == rcx.OK
    assert L.rcx_planes_join_device(h, r + n, n, 4, 4096, r + 2 * n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[:n], noise[:n]) and np.array_equal(got[n: 2 * n], y) and np.array_equal(got[2 * n:], noise[:n])
    room.check(3 * n, "room")


def test_needs_no_reserve_and_takes_any_stream(noise):
    fresh = rcx.Context(0)
    try:
        x = noise[: 5 * 8192 + 77]
        src, dst = Guarded(len(x), 1, x, salt=1), Guarded(len(x), 3, salt=2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        planes.split_device(fresh, src.view, 2, 4096, dst.view, stream=side)
        assert fresh.sync_status(stream=side, raise_on_error=False)[0] == rcx.OK
        dst.check(len(x), "dst")
        assert np.array_equal(dst.view.cpu().numpy(), pc.split_numpy(x, 2, 4096))
        assert fresh.scratch_bytes() == 0  # nothing was allocated for it
    finally:
        fresh.close()


# ---- the streams are the oracle's ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_streams(oracle, bf16):
    """Per (n, block): the bf16 bytes, and for every coder the oracle's compacted streams of their planes (computed once)."""
    out = {}
    for n, block in ((300_000, 4096), (3 * 2 * 65536 + 1001, 65536)):
        x = bf16[:n]
        y = pc.split_numpy(x, 2, block)
        out[(n, block)] = (x, y, {coder: oracle.compact(*oracle.encode_blocks(y, block, coder=coder, threads=8)) for coder in CODERS})
    return out


@pytest.mark.parametrize("coder", CODERS)
def test_typed_container_streams_are_the_oracles(ctx, split_streams, coder):
    for (n, block), (x, y, want) in split_streams.items():
        payload, offsets = want[coder]
        for checksum in (False, True):
            blob = container.pack_typed(x.tobytes(), 2, block, coder, ctx, checksum=checksum)
            c = container.parse_typed(blob)
            assert (c["coder"], c["block"], c["n"], c["width"], c["nblocks"]) == (coder, block, n, 2, rcx.block_count(n, block))
            assert np.array_equal(c["offsets"], offsets), (n, block, coder)
            assert np.array_equal(c["payload"], payload), (n, block, coder)
            if checksum:  # of the split text, what the coder saw
                assert np.array_equal(c["crcs"], [zlib.crc32(y[at: at + block].tobytes()) for at in range(0, n, block)])
            else:
                assert c["crcs"] is None
            assert container.unpack_typed(blob, ctx) == x.tobytes()


# ---- containers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_round_trips(ctx, noise, coder):
    fp32 = pc.randn_bytes("fp32", 1 << 18)[0]
    for data, width, block in ((fp32[: 3 * 4 * 4096 + 1003], 4, 4096), (fp32[:70_001], 8, 4096), (noise[:33], 2, 16), (fp32[:5], 8, 65536), (b"", 4, 4096)):
        data = bytes(data)
        assert len(data) % width or not data
        for checksum in (False, True):
            blob = container.pack_typed(data, width, block, coder, ctx, checksum=checksum)
            assert container.unpack_typed(blob, ctx) == data, (len(data), width, block, checksum)
            assert container.unpack_typed(blob, ctx, verify=False) == data


def test_a_gpu_tensor_gives_the_blob_of_its_bytes(ctx):
    torch.manual_seed(7)
    values = torch.randn(50_001) * 0.02
    for t in (values.to(torch.bfloat16), values, torch.randint(0, 50_000, (20_001,), dtype=torch.int64)):
        raw = t.view(torch.uint8).numpy().tobytes()
        width = t.element_size()
        want = container.pack_typed(raw, width, 4096, 0, ctx, checksum=True)
        assert container.parse_typed(want)["width"] == width
        assert container.pack_typed(t.cuda(), None, 4096, 0, ctx, checksum=True) == want          # where it lies
        assert container.pack_typed(t, None, 4096, 0, ctx, checksum=True) == want                 # a CPU tensor
        assert container.pack_typed(t.numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).numpy(), None, 4096, 0, ctx, checksum=True) == want
        assert container.unpack_typed(want, ctx) == raw
    with pytest.raises(container.ContainerError):
        container.pack_typed(torch.zeros(64, dtype=torch.uint8, device="cuda"), None, 4096, 0, ctx)


RANGE_W, RANGE_B = 4, 4096
RANGE_S = RANGE_W * RANGE_B
RANGE_N = 5 * RANGE_S + 9001  # five whole superblocks and a ragged one of 2250 elements and a byte: 23 blocks


def spy_on_picks(monkeypatch, ctx):
    """Every pick the item decode call is handed from here on, in a list."""
    seen, real = [], ctx.decode_items_device

    def decode_items_device(*a, pick=None, **kw):
        seen.append([int(k) for k in pick])
        return real(*a, pick=pick, **kw)

    monkeypatch.setattr(ctx, "decode_items_device", decode_items_device)
    return seen


RANGES = (  # (start, stop, the blocks that cover the range's superblocks)
    (100, 5000, range(0, 4)),                                   # inside one superblock
    (RANGE_S - 10, RANGE_S + 700, range(0, 8)),                 # across a superblock border
    (2 * RANGE_S, 3 * RANGE_S, range(8, 12)),                   # exactly one
    (5 * RANGE_S - 10, 5 * RANGE_S + 5000, range(16, 23)),      # into the ragged last one
    (RANGE_N - 1, RANGE_N, range(20, 23)),                      # its tail byte
    (0, RANGE_N, range(0, 23)),
)


@pytest.mark.parametrize("checksum", (False, True))
def test_ranges_decode_only_the_covering_blocks(ctx, monkeypatch, checksum):
    data = pc.randn_bytes("fp32", 1 << 17)[0][:RANGE_N].tobytes()
    blob = container.pack_typed(data, RANGE_W, RANGE_B, 0, ctx, checksum=checksum)
    assert container.parse_typed(blob)["nblocks"] == 23
    seen = spy_on_picks(monkeypatch, ctx)
    for start, stop, blocks in RANGES:
        assert container.unpack_typed_range(blob, start, stop, ctx) == data[start:stop], (start, stop)
        assert seen[-1] == list(blocks), (start, stop, seen[-1])
    assert len(seen) == len(RANGES)
    assert container.unpack_typed_range(blob, 777, 777, ctx) == b"" and len(seen) == len(RANGES)
    for start, stop in ((-1, 5), (5, 4), (0, RANGE_N + 1)):
        with pytest.raises(container.ContainerError):
            container.unpack_typed_range(blob, start, stop, ctx)


def silent_flip(oracle, stream, good, block):
    """A single-bit flip near the end of `stream` that the oracle decodes completely, to other bytes -> (byte, bit)."""
    for back in range(6, 70):
        for bit in (0x01, 0x10, 0x80):
            s = stream.copy()
            s[len(s) - back] ^= bit
            ok, out = oracle_decode_one(oracle, s, len(good), 0, block)
            if ok and not np.array_equal(out, good):
                return len(s) - back, bit
    return None


def test_a_flipped_bit_names_its_block(ctx, oracle):
    data = pc.randn_bytes("fp32", 1 << 17)[0][:RANGE_N].tobytes()
    split = pc.split_numpy(np.frombuffer(data, np.uint8), RANGE_W, RANGE_B)
    blob = container.pack_typed(data, RANGE_W, RANGE_B, 0, ctx, checksum=True)
    c = container.parse_typed(blob)
    payload_at = len(blob) - len(c["payload"])
    crc_at = payload_at - 4 * c["nblocks"]
    for bad_block in (9, 22):  # plane 1 of superblock 2; the last block of the ragged superblock
        damaged = [bytearray(blob)]
        damaged[0][crc_at + 4 * bad_block + 1] ^= 0x04  # a bit of the block's stored checksum
        stream = np.array(c["payload"][int(c["offsets"][bad_block]): int(c["offsets"][bad_block + 1])])
        at = silent_flip(oracle, stream, split[bad_block * RANGE_B: (bad_block + 1) * RANGE_B], RANGE_B)
        assert at is not None, "no flip that the oracle decodes to other bytes"
        damaged.append(bytearray(blob))
        damaged[1][payload_at + int(c["offsets"][bad_block]) + at[0]] ^= at[1]  # a bit of its stream: decodes, to other bytes
        first, last = bad_block // RANGE_W * RANGE_S, min((bad_block // RANGE_W + 1) * RANGE_S, RANGE_N)
        for k, bad in enumerate(bytes(b) for b in damaged):
            with pytest.raises(container.ChecksumError) as e:
                container.unpack_typed(bad, ctx)
            assert (e.value.kind, e.value.index) == ("block", bad_block)
            with pytest.raises(container.ChecksumError) as e:
                container.unpack_typed_range(bad, first + 5, last - 1, ctx)
            assert e.value.index == bad_block  # the container's block, not its place among the picked ones
            # a range that does not touch the bad block's superblock; and nobody asked: the bytes as they decode
            assert container.unpack_typed_range(bad, 100, first, ctx) == data[100:first]
            got = container.unpack_typed(bad, ctx, verify=False)
            assert (got == data) == (k == 0) and len(got) == len(data)
            assert container.unpack_typed_range(bad, first + 5, last - 1, ctx, verify=False) == got[first + 5: last - 1]
    assert container.unpack_typed(blob, ctx) == data


# ---- capture -------------------------------------------------------------------------------------------------------------------
def test_split_encode_and_decode_join_replay_from_a_graph(ctx, oracle):
    width, block = 2, 65536
    n = 16 * width * block + 100
    data = pc.randn_bytes("bf16", 1 << 22)[0][:n]
    data2 = pc.randn_bytes("bf16", 1 << 22, seed=99)[0][:n]
    want = [oracle.compact(*oracle.encode_blocks(pc.split_numpy(d, width, block), block, threads=8)) for d in (data, data2)]
    nblocks = rcx.block_count(n, block)
    src = torch.from_numpy(data).cuda()
    mid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.reserve(n, block)

    def encode():
        planes.split_device(ctx, src, width, block, mid)
        ctx.encode_blocks_device(mid, block, dst, offs)

    def decode():
        ctx.decode_blocks_device(dst, dst.numel(), offs, n, block, back)
        planes.join_device(ctx, back, width, block, out)

    def check(k):
        payload, offsets = want[k]
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), offsets)
        assert np.array_equal(dst[: int(offsets[-1])].cpu().numpy(), payload) and torch.equal(out, src)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        encode()
        decode()
        ctx.sync_status()
    side.synchronize()
    check(0)
    # capture each chain once, replay on new input
    g_enc, g_dec = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_enc):
        encode()
    with torch.cuda.graph(g_dec):
        decode()
    src.copy_(torch.from_numpy(data2).cuda())
    out.zero_()
    g_enc.replay()
    g_dec.replay()
    torch.cuda.synchronize()
    ctx.sync_status()
    check(1)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def run_cli(*a):
    return subprocess.run([sys.executable, "-m", "cpprcoder_amd", *a], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=600)


def test_cli_round_trip_by_planes(tmp_path, bf16):
    src = tmp_path / "in.bf16"
    src.write_bytes(bf16[:300_001].tobytes())
    r = run_cli("c", "--planes", "2", "--crc", "-b", "16384", str(src), str(tmp_path / "out.rcxt"))
    assert r.returncode == 0, r.stderr
    c = container.parse_typed((tmp_path / "out.rcxt").read_bytes())
    assert c["width"] == 2 and c["crcs"] is not None and c["block"] == 16384
    r = run_cli("d", str(tmp_path / "out.rcxt"), str(tmp_path / "back.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "back.bin").read_bytes() == src.read_bytes()
    r = run_cli("t", "--planes", "2", str(src))
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
