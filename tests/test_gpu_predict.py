"""The delta predictor on the GPU (include/rcx_predict.h; csrc/rcx_predict.hpp) against its numpy restatement
(tests/predict_cases.py), and the typed container with a predictor against the CPU oracle.

The inverse kernel gives a wave whole superblocks and walks each one in tiles of 64 units = 1024 elements, carrying the
running element; the last m % 16 elements end the same chain.  The blocks sit on both sides of every border of that: 16, 48
and 100 (a tile with idle lanes, planes off 16-byte borders), 1024 and 1040 (one tile, and a unit more), 4096 and 4112
(four tiles, and a unit more), 12304 (twelve tiles and a unit); n around one element, one unit and one superblock, with a
ragged fourth superblock; source and destination at every offset of (0, 1, 3, 8, 15), every buffer guarded; random
bytes (every sum wraps), the elements -k (every difference all 0xFF: the carry runs through every byte) and, for width 8, a
ramp across 2^32; 8 MiB + 5 bytes at 64 KiB blocks, where the forward kernel's fixed grid loops; and buffers with more
superblocks than the inverse kernel's grid has waves (32 a compute unit, read from the device), where that grid
loops, a wave owns several superblocks and loads the first row of its next one ahead.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import planes_cases as pc
import predict_cases as pr
from cpprcoder_amd import container, predict, rcx
from gpu_support import CODERS, Guarded, ctx, oracle_decode_one, run_filter  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20252).randint(0, 256, (8 << 20) + 64, dtype=np.uint8)


def run(ctx, join, x, width, block, pred, src_offset=0, dst_offset=0):
    """gpu_support.run_filter of one predictor call."""
    fn = predict.join_device if join else predict.split_device
    return run_filter(ctx, lambda src, dst: fn(ctx, src, width, block, pred, dst), f"{'join' if join else 'split'} w={width} B={block} pred={pred}", x,
                      src_offset, dst_offset)


# ---- the kernels against numpy ----------------------------------------------------------------------------------------------
KERNEL_RUNS = [(w, p, kind) for w in pr.WIDTHS for p in pr.PREDS for kind in pr.KINDS if kind != "ramp" or w == 8]


@pytest.mark.parametrize("width,pred,kind", KERNEL_RUNS)
def test_split_and_join_against_numpy(ctx, noise, width, pred, kind):
    cases = [c for c in pr.kernel_cases() if c[0] == width]
    assert len(cases) == 12 * len(pr.BLOCKS)
    for k, (_, block, n, so, do) in enumerate(cases):
        x = pr.kernel_data(kind, width, n, noise[k:])
        y = pr.split_numpy(x, width, block, pred)
        got = run(ctx, False, x, width, block, pred, so, do)
        bad = np.flatnonzero(got != y)
        assert len(bad) == 0, ("split", width, block, pred, kind, n, so, do, bad[:8])
        back = run(ctx, True, y, width, block, pred, do, so)
        bad = np.flatnonzero(back != x)
        assert len(bad) == 0, ("join", width, block, pred, kind, n, do, so, bad[:8])


@pytest.mark.parametrize("width", pr.WIDTHS)
def test_no_predictor_is_the_plane_filter(ctx, noise, width):
    for block, n in ((100, 5 * width * 100 + 3), (4096, 3 * width * 4096 + 5)):
        x = noise[7: 7 + n]
        y = pc.split_numpy(x, width, block)
        assert np.array_equal(run(ctx, False, x, width, block, predict.NONE, 1, 3), y)
        assert np.array_equal(run(ctx, True, y, width, block, predict.NONE, 3, 1), x)


@pytest.mark.parametrize("width", pr.WIDTHS)
def test_eight_mebibytes_and_five_bytes(ctx, noise, width):
    n, block = (8 << 20) + 5, 65536
    x = noise[3: 3 + n]
    for pred in pr.PREDS:
        y = pr.split_numpy(x, width, block, pred)
        assert np.array_equal(run(ctx, False, x, width, block, pred), y), pred
        assert np.array_equal(run(ctx, True, y, width, block, pred), x), pred


@pytest.mark.parametrize("case", range(4))
def test_more_superblocks_than_the_inverse_grid_has_waves(ctx, case):
    waves = 32 * torch.cuda.get_device_properties(0).multi_processor_count  # typed_launch's grid for the inverse with a predictor
    width, block, n = pr.looping_cases(waves)[case]
    assert -(-n // (width * block)) > waves
    x = np.random.RandomState(77 + case).randint(0, 256, n, dtype=np.uint8)
    for pred in (pr.ZIGZAG,) if case == 3 else pr.PREDS:  # (the largest one: the inverse only, it is the kernel this is about)
        y = pr.split_numpy(x, width, block, pred)
        if case != 3:
            assert np.array_equal(run(ctx, False, x, width, block, pred, 1, 8), y), (width, block, pred)
        back = run(ctx, True, y, width, block, pred, 3, 0)
        bad = np.flatnonzero(back != x)
        assert len(bad) == 0, ("join", width, block, pred, n, bad[:8], bad[:8] // (width * block))


def test_host_buffer_calls(ctx, noise):
    for width, block, n, pred in ((2, 4096, 3 * 8192 + 5, predict.DELTA), (4, 100, 1234, predict.ZIGZAG), (8, 65536, (1 << 20) + 3, predict.ZIGZAG),
                                  (8, 1040, 50_001, predict.DELTA), (4, 16, 0, predict.DELTA), (2, 48, 777, predict.NONE)):
        x = noise[:n]
        y = predict.split(ctx, x, width, block, pred)
        assert y == pr.split_numpy(x, width, block, pred).tobytes(), (width, block, n, pred)
        assert predict.join(ctx, y, width, block, pred) == x.tobytes(), (width, block, n, pred)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(ctx, noise):
    L, h = predict.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    src = Guarded(n, 0, noise[:n], salt=1)
    dst = Guarded(n, 0, salt=2)
    room = Guarded(3 * n, 0, noise[: 3 * n], salt=3)  # one allocation for the overlapping and the adjacent ranges
    s, d, r = src.view.data_ptr(), dst.view.data_ptr(), room.view.data_ptr()
    host_out = np.full(n, 0xA5, np.uint8)
    for fn in (L.rcx_predict_split_device, L.rcx_predict_join_device):
        for pred in (0, 1, 2):  # nothing to do
            assert fn(h, s, 0, 2, 4096, pred, d, stream) == rcx.OK and fn(h, None, 0, 8, 16, pred, None, stream) == rcx.OK
        for st in (fn(h, s, n, 4, 4096, 3, d, stream), fn(h, s, n, 4, 4096, 255, d, stream), fn(h, s, n, 4, 4096, 0xFFFFFFFF, d, stream),  # the predictor
                   fn(h, s, 0, 4, 4096, 3, d, stream),                                                   # ... also with nothing to do
                   fn(h, s, n, 0, 4096, 1, d, stream), fn(h, s, n, 1, 4096, 1, d, stream), fn(h, s, n, 3, 4096, 2, d, stream), fn(h, s, n, 16, 4096, 1, d, stream),
                   fn(h, s, n, 6, 4096, 2, d, stream),                                                   # the width
                   fn(h, s, n, 4, 15, 1, d, stream), fn(h, s, n, 4, 0, 2, d, stream), fn(h, s, n, 4, rcx.MAX_BLOCK + 1, 1, d, stream),  # the block
                   fn(h, s, 0, 3, 4096, 1, d, stream), fn(h, s, 0, 4, 15, 2, d, stream),
                   fn(h, None, n, 4, 4096, 1, d, stream), fn(h, s, n, 4, 4096, 2, None, stream),          # null pointers
                   fn(None, s, n, 4, 4096, 1, d, stream),
                   fn(h, r, n, 4, 4096, 1, r, stream), fn(h, r, n, 4, 4096, 2, r + 1, stream), fn(h, r + 1, n, 4, 4096, 1, r, stream),  # overlaps
                   fn(h, r, n, 4, 4096, 2, r + n - 1, stream), fn(h, r + n - 1, n, 4, 4096, 1, r, stream), fn(h, r, n, 4, 4096, 0, r + 1, stream)):
            assert st == rcx.E_ARG
    for fn in (L.rcx_predict_split, L.rcx_predict_join):
        for st in (fn(h, noise.ctypes.data, n, 4, 4096, 3, host_out.ctypes.data), fn(h, noise.ctypes.data, n, 5, 4096, 1, host_out.ctypes.data),
                   fn(h, noise.ctypes.data, n, 4, 8, 2, host_out.ctypes.data), fn(h, None, n, 4, 4096, 1, host_out.ctypes.data),
                   fn(h, noise.ctypes.data, n, 4, 4096, 1, None), fn(h, noise.ctypes.data, n, 4, 4096, 2, noise.ctypes.data + 100)):
            assert st == rcx.E_ARG
        assert fn(h, None, 0, 4, 4096, 1, None) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for g, what in ((src, "src"), (dst, "dst"), (room, "room")):
        g.check(0, what)  # not a byte changed anywhere
    assert bool((host_out == 0xA5).all())
    # ranges that touch are apart: the second third of the allocation from its first, and the third from the second
    y = pr.split_numpy(noise[:n], 4, 4096, predict.ZIGZAG)
    assert L.rcx_predict_split_device(h, r, n, 4, 4096, 2, r + n, stream) == rcx.OK
    assert L.rcx_predict_join_device(h, r + n, n, 4, 4096, 2, r + 2 * n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[:n], noise[:n]) and np.array_equal(got[n: 2 * n], y) and np.array_equal(got[2 * n:], noise[:n])
    room.check(3 * n, "room")


def test_needs_no_reserve_and_takes_any_stream(noise):
    fresh = rcx.Context(0)
    try:
        x = noise[: 5 * 8192 + 77]
        y = pr.split_numpy(x, 2, 4096, predict.DELTA)
        src, mid, dst = Guarded(len(x), 1, x, salt=1), Guarded(len(x), 3, salt=2), Guarded(len(x), 8, salt=3)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        predict.split_device(fresh, src.view, 2, 4096, predict.DELTA, mid.view, stream=side)
        predict.join_device(fresh, mid.view, 2, 4096, predict.DELTA, dst.view, stream=side)
        assert fresh.sync_status(stream=side, raise_on_error=False)[0] == rcx.OK
        mid.check(len(x), "mid")
        dst.check(len(x), "dst")
        assert np.array_equal(mid.view.cpu().numpy(), y) and np.array_equal(dst.view.cpu().numpy(), x)
        assert fresh.scratch_bytes() == 0  # nothing was allocated for it
    finally:
        fresh.close()


# ---- the streams are the oracle's ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predicted_streams(oracle):
    """Per shape: the integers, their predicted planes, and for every coder the oracle's compacted streams of those (once)."""
    out = []
    for name, pred, n, block in (("random_walk", pr.ZIGZAG, 300_000, 4096), ("sorted_keys", pr.DELTA, 3 * 8 * 65536 + 1001, 65536)):
        x, width = pr.integer_bytes(name, 1 << 21)
        x = x[:n]
        y = pc.split_numpy(pr.predict_numpy(x, width, block, pred), width, block)
        out.append((x, y, width, pred, n, block, {coder: oracle.compact(*oracle.encode_blocks(y, block, coder=coder, threads=8)) for coder in CODERS}))
    return out


@pytest.mark.parametrize("coder", CODERS)
def test_container_streams_are_the_oracles(ctx, predicted_streams, coder):
    for x, y, width, pred, n, block, want in predicted_streams:
        payload, offsets = want[coder]
        for checksum in (False, True):
            blob = container.pack_typed(x.tobytes(), width, block, coder, ctx, checksum=checksum, predict=pr.NAMES[pred])
            c = container.parse_typed(blob)
            assert blob[4] == 2 and (c["coder"], c["block"], c["n"], c["width"], c["pred"], c["nblocks"]) == (coder, block, n, width, pred, rcx.block_count(n, block))
            assert np.array_equal(c["offsets"], offsets), (n, block, coder)
            assert np.array_equal(c["payload"], payload), (n, block, coder)
            if checksum:  # of the predicted and split text, what the coder saw
                assert np.array_equal(c["crcs"], [zlib.crc32(y[at: at + block].tobytes()) for at in range(0, n, block)])
            else:
                assert c["crcs"] is None
            assert container.unpack_typed(blob, ctx) == x.tobytes()


def test_without_a_predictor_the_container_is_what_it_was(ctx):
    x, width = pr.integer_bytes("signal", 1 << 17)
    x = x[:100_001]
    blob = container.pack_typed(x.tobytes(), width, 4096, 0, ctx, checksum=True)
    assert blob[4] == 1 and blob[29] == 0 and container.pack_typed(x.tobytes(), width, 4096, 0, ctx, checksum=True, predict=None) == blob
    delta = container.pack_typed(x.tobytes(), width, 4096, 0, ctx, checksum=True, predict="delta")
    assert delta[4] == 2 and delta[29] == 1 and len(delta) < len(blob)  # (what it is for)
    assert container.unpack_typed(blob, ctx) == container.unpack_typed(delta, ctx) == x.tobytes()


# ---- containers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_round_trips(ctx, noise, coder):
    walk = pr.integer_bytes("random_walk", 1 << 18)[0]
    keys = pr.integer_bytes("sorted_keys", 1 << 18)[0]
    for data, width, block, predict_ in ((walk[: 3 * 4 * 4096 + 1003], 4, 4096, "zigzag"), (keys[:70_001], 8, 4096, "delta"), (noise[:33], 2, 16, "zigzag"),
                                         (keys[:5], 8, 65536, "delta"), (walk[:4 * 1040 * 2 + 6], 4, 1040, "delta"), (b"", 4, 4096, "zigzag")):
        data = bytes(data)
        assert len(data) % width or not data
        for checksum in (False, True):
            blob = container.pack_typed(data, width, block, coder, ctx, checksum=checksum, predict=predict_)
            assert container.parse_typed(blob)["pred"] == container.PREDICTORS[predict_]
            assert container.unpack_typed(blob, ctx) == data, (len(data), width, block, checksum)
            assert container.unpack_typed(blob, ctx, verify=False) == data


def test_a_gpu_tensor_gives_the_blob_of_its_bytes(ctx):
    torch.manual_seed(7)
    steps = torch.randint(-100, 101, (50_001,))
    for t, predict_ in ((torch.cumsum(steps, 0).to(torch.int32), "zigzag"), (torch.cumsum(steps.abs(), 0), "delta"), (torch.cumsum(steps, 0).to(torch.int16), "zigzag")):
        raw = t.view(torch.uint8).numpy().tobytes()
        width = t.element_size()
        want = container.pack_typed(raw, width, 4096, 0, ctx, checksum=True, predict=predict_)
        c = container.parse_typed(want)
        assert c["width"] == width and c["pred"] == container.PREDICTORS[predict_]
        assert container.pack_typed(t.cuda(), None, 4096, 0, ctx, checksum=True, predict=predict_) == want   # where it lies
        assert container.pack_typed(t, None, 4096, 0, ctx, checksum=True, predict=predict_) == want          # a CPU tensor
        assert container.pack_typed(t.numpy(), None, 4096, 0, ctx, checksum=True, predict=predict_) == want
        assert container.unpack_typed(want, ctx) == raw


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


@pytest.fixture(scope="module")
def range_data():
    return pr.integer_bytes("random_walk", 1 << 17)[0][:RANGE_N].tobytes()


@pytest.mark.parametrize("checksum", (False, True))
def test_ranges_decode_only_the_covering_blocks(ctx, monkeypatch, range_data, checksum):
    data = range_data
    blob = container.pack_typed(data, RANGE_W, RANGE_B, 0, ctx, checksum=checksum, predict="zigzag")
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


def test_a_flipped_bit_names_its_block(ctx, oracle, range_data):
    data = range_data
    split = pr.split_numpy(np.frombuffer(data, np.uint8), RANGE_W, RANGE_B, pr.DELTA)
    blob = container.pack_typed(data, RANGE_W, RANGE_B, 0, ctx, checksum=True, predict="delta")
    c = container.parse_typed(blob)
    payload_at = len(blob) - len(c["payload"])
    crc_at = payload_at - 4 * c["nblocks"]
    for bad_block in (8, 22):  # plane 0 of superblock 2; the last block of the ragged superblock
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
            # the damage stays inside its superblock: the predictor restarts at the border
            assert got[:first] == data[:first] and got[last:] == data[last:]
            assert container.unpack_typed_range(bad, first + 5, last - 1, ctx, verify=False) == got[first + 5: last - 1]
    assert container.unpack_typed(blob, ctx) == data


# ---- capture -------------------------------------------------------------------------------------------------------------------
def test_split_encode_and_decode_join_replay_from_a_graph(ctx, oracle):
    width, block, pred = 4, 65536, predict.ZIGZAG
    n = 8 * width * block + 100
    data = pr.integer_bytes("random_walk", 1 << 22)[0][:n]
    data2 = pr.integer_bytes("random_walk", 1 << 22, seed=99)[0][:n]
    want = [oracle.compact(*oracle.encode_blocks(pr.split_numpy(d, width, block, pred), block, threads=8)) for d in (data, data2)]
    nblocks = rcx.block_count(n, block)
    src = torch.from_numpy(data).cuda()
    mid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.reserve(n, block)

    def encode():
        predict.split_device(ctx, src, width, block, pred, mid)
        ctx.encode_blocks_device(mid, block, dst, offs)

    def decode():
        ctx.decode_blocks_device(dst, dst.numel(), offs, n, block, back)
        predict.join_device(ctx, back, width, block, pred, out)

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


def test_cli_round_trip_with_a_predictor(tmp_path):
    src = tmp_path / "in.i64"
    src.write_bytes(pr.integer_bytes("csr_offsets", 1 << 19)[0][:300_001].tobytes())
    r = run_cli("c", "--planes", "8", "--predict", "delta", "--crc", "-b", "16384", str(src), str(tmp_path / "out.rcxt"))
    assert r.returncode == 0, r.stderr
    c = container.parse_typed((tmp_path / "out.rcxt").read_bytes())
    assert c["width"] == 8 and c["pred"] == 1 and c["crcs"] is not None and c["block"] == 16384
    r = run_cli("d", str(tmp_path / "out.rcxt"), str(tmp_path / "back.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "back.bin").read_bytes() == src.read_bytes()
    r = run_cli("t", "--planes", "8", "--predict", "zigzag", str(src))
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    r = run_cli("c", "--predict", "delta", str(src), str(tmp_path / "no.rcxt"))
    assert r.returncode == 2 and not (tmp_path / "no.rcxt").exists()
