"""Residuals against a base on the GPU (include/rcx_base.h; csrc/rcx_base.hpp) against the numpy twin of the package
(cpprcoder_amd/base.py), and the RCXD container against the CPU oracle.

The kernel is elementwise; its borders are those of the plane kernel -- units of 16 elements, superblocks, the rest elements and
tail bytes behind the units -- and one of its own: a workgroup takes RCX_BASE_U4 / (2 * width) rows of 256 units a STEP, without
bounds tests while a whole step is left (rcx_base_k: `first + STEP <= total`) and with them in the last one.  base_cases.sizes
therefore adds exactly one step, and a step, a unit, an element and a byte more, to n around one element, one unit and one
superblock with a ragged fourth; the blocks are 16, 48, 100, 4096 and 4112; source, base and destination each sit at every
offset of (0, 1, 3, 8, 15), cycling independently, every buffer guarded.  Width 1 has no superblocks: its rest is the last
n % 16 bytes, which workgroup 0 takes (`blockIdx.x == 0 && i < n`).  Data: random bytes, the source equal to the base, the
source one below the base in every element (the borrow runs through every byte) and, for width 8, pairs on both sides of 2^32.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import base_cases as bc
import large_cases as lc
from cpprcoder_amd import base, container, rcx
from gpu_support import CODERS, Guarded, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20261).randint(0, 256, (17 << 20) + 64, dtype=np.uint8)


def run(ctx, join, x, ref, width, block, op, src_offset=0, ref_offset=0, dst_offset=0):
    """One device call with all three buffers guarded -> the n bytes written; source and base are unchanged, and nothing but
    the n bytes of the destination is written."""
    n = len(x)
    src, b, dst = Guarded(n, src_offset, x, salt=1), Guarded(n, ref_offset, ref, salt=2), Guarded(n, dst_offset, salt=3)
    assert n == 0 or all(g.view.data_ptr() % 16 == o % 16 for g, o in ((src, src_offset), (b, ref_offset), (dst, dst_offset)))
    (base.join_device if join else base.split_device)(ctx, src.view, b.view, width, block, op, dst.view)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    what = f"{'join' if join else 'split'} w={width} B={block} op={op} n={n} offsets {src_offset}, {ref_offset}, {dst_offset}"
    src.check(0, what + ": src")
    b.check(0, what + ": base")
    dst.check(n, what + ": dst")
    return dst.view.cpu().numpy()


def both_ways(ctx, x, ref, width, block, op, offsets=(0, 0, 0), what=()):
    y = base.split_numpy(x, ref, width, block, op)
    got = run(ctx, False, x, ref, width, block, op, *offsets)
    bad = np.flatnonzero(got != y)
    assert len(bad) == 0, ("split", width, block, op, len(x), offsets, what, bad[:8])
    so, bo, do = offsets
    back = run(ctx, True, y, ref, width, block, op, do, bo, so)
    bad = np.flatnonzero(back != x)
    assert len(bad) == 0, ("join", width, block, op, len(x), offsets, what, bad[:8])


# ---- the kernels against numpy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", bc.OPS, ids=[bc.NAMES[op] for op in bc.OPS])
@pytest.mark.parametrize("width", bc.WIDTHS)
def test_split_and_join_against_numpy(ctx, noise, width, op):
    cases = [c for c in bc.kernel_cases() if c[0] == width]
    assert len(cases) >= 10 * len(bc.BLOCKS)  # (width 1: an element is a byte, two sizes of the list coincide)
    for k, (_, block, n, so, bo, do) in enumerate(cases):
        x, ref = bc.kernel_data("random", width, n, noise[k:])
        both_ways(ctx, x, ref, width, block, op, (so, bo, do))
        if n == 3 * width * block + 5 and block in (100, 4112):  # a ragged fourth superblock, rest elements, tail bytes
            for kind in bc.KINDS[1:]:
                if kind != "straddle" or width == 8:
                    x, ref = bc.kernel_data(kind, width, n, noise[k:])
                    both_ways(ctx, x, ref, width, block, op, (do, so, bo), kind)


@pytest.mark.parametrize("width", bc.WIDTHS)
def test_eight_mebibytes_and_five_bytes(ctx, noise, width):
    n, block = (8 << 20) + 5, 65536
    x, ref = bc.kernel_data("random", width, n, noise[3:])
    for op in bc.OPS:
        both_ways(ctx, x, ref, width, block, op)


@pytest.mark.parametrize("width", (1, 2))
def test_more_units_than_the_grid_takes_in_one_turn(ctx, noise, width):
    """base_grid is four workgroups a compute unit, and a workgroup takes a step a turn: on a device with 256 compute units that
    is 32 MiB, so 8 MiB do not make the grid loop.  Here n is that capacity (from the device's count), a step, a unit and 5 bytes
    more: every workgroup takes a second turn or finds none, and one takes the step with the bounds tests in its second turn."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * cus * bc.step_bytes(width) + bc.step_bytes(width) + 16 * width + 5
    x, ref = np.resize(noise[: (8 << 20) + 13], n), np.resize(noise[8 << 20: (16 << 20) + 7], n)
    both_ways(ctx, x, ref, width, 65536, base.SUBZZ, (1, 8, 3))


def test_host_buffer_calls(ctx, noise):
    for width, block, n, op in ((2, 4096, 3 * 8192 + 5, base.SUBZZ), (4, 100, 1234, base.SUB), (8, 65536, (1 << 20) + 3, base.SUBZZ), (1, 1040, 50_001, base.SUBZZ),
                                (1, 16, 15, base.SUB), (4, 16, 0, base.XOR), (1, 4096, 0, base.SUBZZ), (2, 48, 777, base.XOR)):
        x, ref = bc.kernel_data("random", width, n, noise)
        y = base.split(ctx, x, ref, width, block, op)
        assert y == base.split_numpy(x, ref, width, block, op).tobytes(), (width, block, n, op)
        assert base.join(ctx, y, ref, width, block, op) == x.tobytes(), (width, block, n, op)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(ctx, noise):
    L, h = base.lib(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    n = 4096
    src, ref, dst = Guarded(n, 0, noise[:n], salt=1), Guarded(n, 0, noise[n: 2 * n], salt=2), Guarded(n, 0, salt=3)
    room = Guarded(4 * n, 0, noise[: 4 * n], salt=4)  # one allocation for the overlapping and the adjacent ranges
    s, b, d, r = src.view.data_ptr(), ref.view.data_ptr(), dst.view.data_ptr(), room.view.data_ptr()
    host_out = np.full(n, 0xA5, np.uint8)
    for fn in (L.rcx_base_split_device, L.rcx_base_join_device):
        for op in (0, 1, 2):  # nothing to do
            assert fn(h, s, b, 0, 2, 4096, op, d, stream) == rcx.OK and fn(h, None, None, 0, 1, 16, op, None, stream) == rcx.OK
        for st in (fn(h, s, b, n, 4, 4096, 3, d, stream), fn(h, s, b, n, 4, 4096, 255, d, stream), fn(h, s, b, n, 1, 4096, 0xFFFFFFFF, d, stream),  # the op
                   fn(h, s, b, 0, 4, 4096, 3, d, stream), fn(h, None, None, 0, 1, 4096, 3, None, stream),                 # ... also with nothing to do
                   fn(h, s, b, n, 0, 4096, 1, d, stream), fn(h, s, b, n, 3, 4096, 1, d, stream), fn(h, s, b, n, 16, 4096, 2, d, stream),
                   fn(h, s, b, n, 6, 4096, 0, d, stream), fn(h, s, b, 0, 3, 4096, 0, d, stream),                         # the width
                   fn(h, s, b, n, 4, 15, 1, d, stream), fn(h, s, b, n, 1, 0, 2, d, stream), fn(h, s, b, n, 4, rcx.MAX_BLOCK + 1, 1, d, stream),
                   fn(h, s, b, 0, 4, 15, 2, d, stream),                                                                   # the block
                   fn(h, None, b, n, 4, 4096, 1, d, stream), fn(h, s, None, n, 4, 4096, 1, d, stream), fn(h, s, b, n, 4, 4096, 2, None, stream),  # null pointers
                   fn(None, s, b, n, 4, 4096, 1, d, stream),
                   fn(h, r, b, n, 4, 4096, 1, r, stream), fn(h, r, b, n, 4, 4096, 2, r + 1, stream), fn(h, r + 1, b, n, 1, 4096, 1, r, stream),  # dst on src
                   fn(h, r, b, n, 4, 4096, 2, r + n - 1, stream), fn(h, r + n - 1, b, n, 4, 4096, 0, r, stream),
                   fn(h, s, r, n, 4, 4096, 1, r, stream), fn(h, s, r, n, 2, 4096, 2, r + 1, stream), fn(h, s, r + 1, n, 4, 4096, 0, r, stream),  # dst on base
                   fn(h, s, r, n, 8, 4096, 2, r + n - 1, stream), fn(h, s, r + n - 1, n, 4, 4096, 1, r, stream)):
            assert st == rcx.E_ARG
    hs, hb = noise.ctypes.data, noise.ctypes.data + 8192
    for fn in (L.rcx_base_split, L.rcx_base_join):
        for st in (fn(h, hs, hb, n, 4, 4096, 3, host_out.ctypes.data), fn(h, hs, hb, n, 5, 4096, 1, host_out.ctypes.data), fn(h, hs, hb, n, 4, 8, 2, host_out.ctypes.data),
                   fn(h, None, hb, n, 4, 4096, 1, host_out.ctypes.data), fn(h, hs, None, n, 4, 4096, 1, host_out.ctypes.data), fn(h, hs, hb, n, 4, 4096, 1, None),
                   fn(h, hs, hb, n, 4, 4096, 2, hs + 100), fn(h, hs, hb, n, 1, 4096, 2, hb + n - 1), fn(h, hs, hb, 0, 4, 4096, 3, host_out.ctypes.data)):
            assert st == rcx.E_ARG
        assert fn(h, None, None, 0, 4, 4096, 1, None) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    for g, what in ((src, "src"), (ref, "base"), (dst, "dst"), (room, "room")):
        g.check(0, what)  # not a byte changed anywhere
    assert bool((host_out == 0xA5).all())
    # ranges that touch are apart: source, base, planes and elements are the four quarters of one allocation; and source and
    # base may overlap, or be the same -- both are only read
    x, rb = noise[:n], noise[n: 2 * n]
    y = base.split_numpy(x, rb, 4, 4096, base.SUBZZ)
    assert L.rcx_base_split_device(h, r, r + n, n, 4, 4096, 2, r + 2 * n, stream) == rcx.OK
    assert L.rcx_base_join_device(h, r + 2 * n, r + n, n, 4, 4096, 2, r + 3 * n, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    got = room.view.cpu().numpy()
    assert np.array_equal(got[: 2 * n], noise[: 2 * n]) and np.array_equal(got[2 * n: 3 * n], y) and np.array_equal(got[3 * n:], x)
    room.check(4 * n, "room")
    assert L.rcx_base_split_device(h, s, s, n, 2, 4096, 1, d, stream) == rcx.OK  # the same buffer: every residual 0
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert not dst.view.cpu().numpy().any()
    half = noise[n // 2: n // 2 + n]  # the source's second half is the base's first
    assert L.rcx_base_split_device(h, r, r + n // 2, n, 2, 4096, 0, d, stream) == rcx.OK
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    assert np.array_equal(dst.view.cpu().numpy(), base.split_numpy(x, half, 2, 4096, base.XOR))
    dst.check(n, "dst")
    src.check(0, "src")


def test_needs_no_reserve_and_takes_any_stream(noise):
    fresh = rcx.Context(0)
    try:
        n = 5 * 8192 + 77
        x, ref = bc.kernel_data("random", 2, n, noise)
        y = base.split_numpy(x, ref, 2, 4096, base.SUBZZ)
        src, b, mid, dst = Guarded(n, 1, x, salt=1), Guarded(n, 15, ref, salt=2), Guarded(n, 3, salt=3), Guarded(n, 8, salt=4)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        base.split_device(fresh, src.view, b.view, 2, 4096, base.SUBZZ, mid.view, stream=side)
        base.join_device(fresh, mid.view, b.view, 2, 4096, base.SUBZZ, dst.view, stream=side)
        assert fresh.sync_status(stream=side, raise_on_error=False)[0] == rcx.OK
        mid.check(n, "mid")
        dst.check(n, "dst")
        b.check(0, "base")
        assert np.array_equal(mid.view.cpu().numpy(), y) and np.array_equal(dst.view.cpu().numpy(), x)
        assert fresh.scratch_bytes() == 0  # nothing was allocated for it
    finally:
        fresh.close()


# ---- capture -------------------------------------------------------------------------------------------------------------------
def test_split_encode_and_decode_join_replay_from_a_graph(ctx, oracle):
    width, block, op = 2, 65536, base.SUBZZ
    n = 8 * width * block + 101
    first, ref1, _ = (a[:n] for a in bc.checkpoint_pair())
    rng = np.random.default_rng(9)
    ref2 = bc.bf16_bytes((rng.standard_normal(n // 2 + 1) * 0.02).astype(np.float32))[:n]
    second = ref2.copy()
    second[::2] += rng.integers(0, 3, len(second[::2])).astype(np.uint8)  # new data against a new base
    want = [oracle.compact(*oracle.encode_blocks(base.split_numpy(d, r, width, block, op), block, threads=8)) for d, r in ((first, ref1), (second, ref2))]
    nblocks = rcx.block_count(n, block)
    src, ref = torch.from_numpy(first.copy()).cuda(), torch.from_numpy(ref1.copy()).cuda()
    mid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.reserve(n, block)

    def encode():
        base.split_device(ctx, src, ref, width, block, op, mid)
        ctx.encode_blocks_device(mid, block, dst, offs)

    def decode():
        ctx.decode_blocks_device(dst, dst.numel(), offs, n, block, back)
        base.join_device(ctx, back, ref, width, block, op, out)

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
    # capture each chain once, replay on new data and a new base
    g_enc, g_dec = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_enc):
        encode()
    with torch.cuda.graph(g_dec):
        decode()
    src.copy_(torch.from_numpy(second).cuda())
    ref.copy_(torch.from_numpy(ref2.copy()).cuda())
    out.zero_()
    g_enc.replay()
    g_dec.replay()
    torch.cuda.synchronize()
    ctx.sync_status()
    check(1)


# ---- past 4 GiB ----------------------------------------------------------------------------------------------------------------
def test_one_case_past_4gib():
    """The recipe of tests/large_cases.py: width 8, subzz, on N = 513 * 8 MiB + 12345 bytes at offsets (1, 3, 8); source and base are
    periodic in 8 MiB, so period 0 and the tail are held to numpy and the later periods to period 0 on the device.  The ragged
    last superblock and its N % 8 tail byte lie past 2^32."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    print(f"holds 17 GiB; free {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB")
    if free < 17 << 30:
        pytest.skip(f"{free / 2**30:.1f} GiB free, the test holds 17 GiB")
    width, op, B, T, K, N = 8, base.SUBZZ, lc.BLOCK, lc.T, lc.K, lc.N
    assert (K * T) % (width * B) == 0 and K * T >= 1 << 32 and lc.TAIL % width
    x, ref = lc.tile("filter"), lc.tile("coder")
    want0, want_tail = base.split_numpy(x, ref, width, B, op), base.split_numpy(lc.tail_of(x), lc.tail_of(ref), width, B, op)
    fresh = rcx.Context(0)
    try:
        src_whole, src = lc.on_device(x, 1)
        ref_whole, b = lc.on_device(ref, 3)
        dst_whole, dst = lc.guarded(N, 8, fill=0x5A)
        base.split_device(fresh, src, b, width, B, op, dst)
        assert fresh.sync_status(raise_on_error=False)[0] == rcx.OK
        assert np.array_equal(dst[:T].cpu().numpy(), want0), "period 0 differs from the numpy twin"
        lc.periodic_equal(dst, T, K, "split")
        assert np.array_equal(dst[K * T:].cpu().numpy(), want_tail), "the ragged last superblock differs from the numpy twin"
        assert lc.guards_intact(dst_whole, dst, fill=0x5A) and lc.guards_intact(src_whole, src) and lc.guards_intact(ref_whole, b)
        lc.periodic_equal(src, T, K, "split source")  # (not written)
        lc.periodic_equal(b, T, K, "base")
        back_whole, back = lc.guarded(N, 15, fill=0x33)
        base.join_device(fresh, dst, b, width, B, op, back)
        assert fresh.sync_status(raise_on_error=False)[0] == rcx.OK
        assert torch.equal(back, src), "join(split(x)) is not x"
        assert lc.guards_intact(back_whole, back, fill=0x33) and lc.guards_intact(dst_whole, dst, fill=0x5A) and lc.guards_intact(ref_whole, b)
        assert fresh.scratch_bytes() == 0
        del src, src_whole, b, ref_whole, dst, dst_whole, back, back_whole
    finally:
        fresh.close()
        torch.cuda.empty_cache()


# ---- containers: the streams are the oracle's ------------------------------------------------------------------------------------
SHAPES = ((2, "subzz", 300_001, 4096), (8, "sub", 3 * 8 * 65536 + 1001, 65536), (1, "xor", 70_003, 4096), (4, "subzz", 50_002, 16384))


@pytest.fixture(scope="module")
def residual_streams(oracle):
    """Per shape: data, base, the numpy residual's split text, and for every coder the oracle's compacted streams of it (once)."""
    out = []
    w2, w, _ = bc.checkpoint_pair()
    now, before = bc.counter_pair(1 << 18)
    for width, op, n, block in SHAPES:
        x, ref = ((now, before) if width == 8 else (w2, w))
        x, ref = x[:n], ref[:n]
        y = base.split_numpy(x, ref, width, block, container.BASE_OPS[op])
        out.append((x, ref, y, width, op, n, block, {coder: oracle.compact(*oracle.encode_blocks(y, block, coder=coder, threads=8)) for coder in CODERS}))
    return out


@pytest.mark.parametrize("coder", CODERS)
def test_container_streams_are_the_oracles(ctx, residual_streams, coder):
    for x, ref, y, width, op, n, block, want in residual_streams:
        payload, offsets = want[coder]
        for checksum in (False, True):
            blob = container.pack_delta(x.tobytes(), ref.tobytes(), width, block, coder, ctx, checksum=checksum, op=op)
            c = container.parse_delta(blob)
            i = c["inner"]
            assert (c["op"], c["width"], c["block"], c["n"], c["kind"]) == (container.BASE_OPS[op], width, block, n, "blocks" if width == 1 else "typed")
            assert (i["coder"], i["nblocks"]) == (coder, rcx.block_count(n, block)) and i.get("pred", 0) == 0
            assert np.array_equal(i["offsets"], offsets), (n, block, coder)
            assert np.array_equal(i["payload"], payload), (n, block, coder)
            assert np.array_equal(c["base_crcs"], [zlib.crc32(ref[at: at + block].tobytes()) for at in range(0, n, block)])  # of the base, in source order
            if checksum:  # of the residual's split text, what the coder saw
                assert np.array_equal(i["crcs"], [zlib.crc32(y[at: at + block].tobytes()) for at in range(0, n, block)])
            else:
                assert i["crcs"] is None
            # an RCXT (RCXB) reader that skips the prefix gets the residual
            inner = blob[c["inner_at"]:]
            if width == 1:
                assert container.unpack(inner, ctx) == y.tobytes()
            else:
                assert container.unpack_typed(inner, ctx) == residual_elements(y, width, block)
            assert container.unpack_delta(blob, ref.tobytes(), ctx) == x.tobytes()


def residual_elements(y, width, block):
    """The residuals themselves: the split text's planes put together again."""
    import planes_cases
    return planes_cases.join_numpy(y, width, block).tobytes()


# ---- containers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_round_trips(ctx, noise, coder):
    w2, w, other = bc.checkpoint_pair(1 << 17)
    now, before = bc.counter_pair(1 << 14)
    for data, ref, width, block, op in ((w2[: 3 * 2 * 4096 + 1003], w[: 3 * 2 * 4096 + 1003], 2, 4096, "subzz"), (now[:70_001], before[:70_001], 8, 4096, "sub"),
                                        (noise[:33], noise[40:73], 2, 16, "xor"), (now[:5], before[:5], 8, 65536, "subzz"),
                                        (w2[: 4 * 1040 * 2 + 6], other[: 4 * 1040 * 2 + 6], 4, 1040, "sub"), (w2[:10_007], w[:10_007], 1, 4096, "subzz"),
                                        (noise[:9000], noise[9000:18000], 1, 100, "sub"), (b"", b"", 4, 4096, "subzz"), (b"", b"", 1, 4096, "xor")):
        data, ref = bytes(data), bytes(ref)
        for checksum in (False, True):
            for stored in (None, True):
                blob = container.pack_delta(data, ref, width, block, coder, ctx, checksum=checksum, stored=stored, op=op)
                c = container.parse_delta(blob)
                assert c["op"] == container.BASE_OPS[op] and (c["inner"]["crcs"] is not None) == checksum
                if stored and data:
                    assert len(c["inner"]["payload"]) <= len(data)  # never past what the coder saw
                assert container.unpack_delta(blob, ref, ctx) == data, (len(data), width, block, checksum, stored)
                assert container.unpack_delta(blob, ref, ctx, verify=False) == data
    # random bytes against random bytes do not shrink: every block ends up stored, and the container says so
    blob = container.pack_delta(bytes(noise[:20_000]), bytes(noise[20_000:40_000]), 4, 4096, coder, ctx, stored=True)
    c = container.parse_delta(blob)
    assert c["inner"]["stored"] is not None and bool(c["inner"]["stored"].all())
    assert container.unpack_delta(blob, bytes(noise[20_000:40_000]), ctx) == bytes(noise[:20_000])


def test_every_kind_of_source_gives_the_same_blob(ctx):
    torch.manual_seed(7)
    w = torch.randn(50_001) * 0.02
    for t, ref, op in (((w + torch.randn(50_001) * 1e-4).to(torch.bfloat16), w.to(torch.bfloat16), "subzz"), (w + torch.randn(50_001) * 1e-5, w, "xor"),
                       (torch.arange(50_001) * 977 + torch.randint(0, 50, (50_001,)), torch.arange(50_001) * 977, "sub"),
                       (torch.randint(0, 256, (50_001,), dtype=torch.uint8), torch.randint(0, 256, (50_001,), dtype=torch.uint8), "subzz")):
        raw, raw_ref = t.view(torch.uint8).numpy().tobytes(), ref.view(torch.uint8).numpy().tobytes()
        width = t.element_size()
        want = container.pack_delta(raw, raw_ref, width, 4096, 0, ctx, checksum=True, op=op)
        c = container.parse_delta(want)
        assert c["width"] == width and c["op"] == container.BASE_OPS[op]
        assert container.pack_delta(t.cuda(), ref.cuda(), None, 4096, 0, ctx, checksum=True, op=op) == want          # where they lie
        assert container.pack_delta(t, ref, None, 4096, 0, ctx, checksum=True, op=op) == want                        # CPU tensors
        assert container.pack_delta(t.cuda(), raw_ref, None, 4096, 0, ctx, checksum=True, op=op) == want             # one of each
        if t.dtype != torch.bfloat16:  # (numpy has no bf16)
            assert container.pack_delta(t.numpy(), ref.numpy(), None, 4096, 0, ctx, checksum=True, op=op) == want
        assert container.unpack_delta(want, raw_ref, ctx) == raw and container.unpack_delta(want, ref.cuda(), ctx) == raw
        assert container.unpack_delta_range(want, ref.cuda(), 5000, 9001, ctx) == raw[5000:9001]
    with pytest.raises(container.ContainerError):
        container.pack_delta(torch.zeros(8, 8).cuda().t(), torch.zeros(8, 8).cuda(), ctx=ctx)  # not contiguous


RANGE_W, RANGE_B = 4, 4096
RANGE_S = RANGE_W * RANGE_B
RANGE_N = 5 * RANGE_S + 9001  # five whole superblocks and a ragged one of 2250 elements and a byte: 23 blocks

RANGES = (  # (start, stop, the blocks that cover the range's superblocks)
    (100, 5000, range(0, 4)),                                   # inside one superblock
    (RANGE_S - 10, RANGE_S + 700, range(0, 8)),                 # across a superblock border
    (2 * RANGE_S, 3 * RANGE_S, range(8, 12)),                   # exactly one
    (5 * RANGE_S - 10, 5 * RANGE_S + 5000, range(16, 23)),      # into the ragged last one
    (RANGE_N - 1, RANGE_N, range(20, 23)),                      # its tail byte
    (0, RANGE_N, range(0, 23)),
)


def spy(monkeypatch, ctx, name, key):
    """Every `key` argument that ctx.<name> is handed from here on, in a list."""
    seen, real = [], getattr(ctx, name)

    def call(*a, **kw):
        seen.append(key(a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ctx, name, call)
    return seen


@pytest.fixture(scope="module")
def range_pair():
    w2, w, _ = bc.checkpoint_pair(1 << 16)
    return w2[:RANGE_N].tobytes(), w[:RANGE_N].tobytes()


@pytest.mark.parametrize("checksum", (False, True))
def test_ranges_decode_only_the_covering_blocks(ctx, monkeypatch, range_pair, checksum):
    data, ref = range_pair
    blob = container.pack_delta(data, ref, RANGE_W, RANGE_B, 0, ctx, checksum=checksum)
    assert container.parse_delta(blob)["inner"]["nblocks"] == 23
    picks = spy(monkeypatch, ctx, "decode_items_device", lambda a, kw: [int(k) for k in kw["pick"]])
    verified = spy(monkeypatch, ctx, "verify_blocks_device", lambda a, kw: int(a[0].numel()))
    for start, stop, blocks in RANGES:
        assert container.unpack_delta_range(blob, ref, start, stop, ctx) == data[start:stop], (start, stop)
        assert picks[-1] == list(blocks), (start, stop, picks[-1])
        assert verified[-1] == sum(min(RANGE_B, RANGE_N - b * RANGE_B) for b in blocks)  # only those blocks of the base
    assert len(picks) == len(RANGES) == len(verified)
    assert container.unpack_delta_range(blob, ref, 777, 777, ctx) == b"" and len(picks) == len(RANGES)
    for start, stop in ((-1, 5), (5, 4), (0, RANGE_N + 1)):
        with pytest.raises(container.ContainerError):
            container.unpack_delta_range(blob, ref, start, stop, ctx)
    # width 1: a superblock is a block
    narrow = container.pack_delta(data, ref, 1, RANGE_B, 0, ctx, checksum=checksum)
    assert container.unpack_delta_range(narrow, ref, RANGE_B - 1, 2 * RANGE_B + 1, ctx) == data[RANGE_B - 1: 2 * RANGE_B + 1] and picks[-1] == [0, 1, 2]


def test_a_flipped_byte_of_the_base_names_its_block(ctx, monkeypatch, range_pair):
    data, ref = range_pair
    blob = container.pack_delta(data, ref, RANGE_W, RANGE_B, 0, ctx, checksum=True)
    decoded = spy(monkeypatch, ctx, "decode_blocks_device", lambda a, kw: 1)
    picks = spy(monkeypatch, ctx, "decode_items_device", lambda a, kw: 1)
    for bad_block, at in ((9, 9 * RANGE_B + 17), (22, RANGE_N - 1), (0, 0)):  # inside superblock 2; the tail byte of the ragged last one; the first byte
        wrong = bytearray(ref)
        wrong[at] ^= 0x20
        wrong = bytes(wrong)
        sb = bad_block // RANGE_W
        first, last = sb * RANGE_S, min((sb + 1) * RANGE_S, RANGE_N)
        before = len(decoded) + len(picks)
        with pytest.raises(container.BaseMismatchError) as e:
            container.unpack_delta(blob, wrong, ctx)
        assert e.value.index == bad_block and isinstance(e.value, container.ContainerError)
        with pytest.raises(container.BaseMismatchError) as e:
            container.unpack_delta_range(blob, wrong, first + 5, last - 1, ctx)
        assert e.value.index == bad_block  # the base's block, not its place among the verified ones
        assert len(decoded) + len(picks) == before  # the base is checked BEFORE anything is decoded
        # a range whose superblocks do not cover the bad block; and nobody asked: wrong bytes inside that superblock only
        lo, hi = (100, first) if first else (last, last + 5000)
        assert container.unpack_delta_range(blob, wrong, lo, hi, ctx) == data[lo:hi]
        got = container.unpack_delta(blob, wrong, ctx, verify=False)
        assert len(got) == len(data) and got[:first] == data[:first] and got[last:] == data[last:]
        if at == RANGE_N - 1:
            assert got == data  # a tail byte of the base is not looked at (include/rcx_base.h): the guard is stricter than the transform
        else:
            assert got[first:last] != data[first:last]
            element = at // RANGE_W * RANGE_W
            assert got[:element] == data[:element] and got[element + RANGE_W:] == data[element + RANGE_W:]  # elementwise: one element, no more
        assert container.unpack_delta_range(blob, wrong, first + 5, last - 1, ctx, verify=False) == got[first + 5: last - 1]
    assert container.unpack_delta(blob, ref, ctx) == data
    # without the table nothing can tell: base_check=False writes none, and the inner checksums pass on the wrong base
    bare = container.pack_delta(data, ref, RANGE_W, RANGE_B, 0, ctx, checksum=True, base_check=False)
    c = container.parse_delta(bare)
    assert c["base_crcs"] is None and c["flags"] == 0 and c["inner_at"] == 24 and len(bare) == len(blob) - 4 * 23
    wrong = bytes([ref[0] ^ 1]) + ref[1:]
    got = container.unpack_delta(bare, wrong, ctx)
    assert got != data and got[RANGE_W:] == data[RANGE_W:]
    for unpack in (lambda: container.unpack_delta(blob, ref[:-1], ctx), lambda: container.unpack_delta_range(blob, ref + b"x", 0, 5, ctx)):
        with pytest.raises(container.ContainerError):
            unpack()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def run_cli(*a):
    return subprocess.run([sys.executable, "-m", "cpprcoder_amd", *a], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=600)


def test_cli_round_trip_against_a_base(tmp_path):
    w2, w, _ = bc.checkpoint_pair(1 << 17)
    src, ref, out, back = tmp_path / "new.bf16", tmp_path / "old.bf16", tmp_path / "out.rcxd", tmp_path / "back.bin"
    src.write_bytes(w2[:200_001].tobytes())
    ref.write_bytes(w[:200_001].tobytes())
    r = run_cli("c", "--planes", "2", "--base", str(ref), "--crc", "-b", "16384", str(src), str(out))
    assert r.returncode == 0, r.stderr
    c = container.parse_delta(out.read_bytes())
    assert (c["width"], c["op"], c["block"]) == (2, 2, 16384) and c["base_crcs"] is not None and c["inner"]["crcs"] is not None
    r = run_cli("d", "--base", str(ref), str(out), str(back))
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == src.read_bytes()
    r = run_cli("t", "--base", str(ref), "--base-op", "sub", str(src))  # without --planes: width 1
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    # the three failure exits: no base, a base of another size, a base of other content -- a message, status 1, nothing written
    short, other = tmp_path / "short.bf16", tmp_path / "other.bf16"
    short.write_bytes(ref.read_bytes()[:-2])
    other.write_bytes(bytes([ref.read_bytes()[0] ^ 1]) + ref.read_bytes()[1:])
    for argv, word in ((["d", str(out)], "--base"), (["d", "--base", str(short), str(out)], "bytes"), (["d", "--base", str(other), str(out)], "base block 0")):
        no = tmp_path / "no.bin"
        r = run_cli(*argv, str(no))
        assert r.returncode == 1 and not no.exists() and word in r.stderr and "nothing written" in r.stderr, (argv, r.stdout, r.stderr)
    r = run_cli("c", "--blksort", "--base", str(ref), str(src), str(tmp_path / "no.rcxd"))
    assert r.returncode == 2 and not (tmp_path / "no.rcxd").exists()
