"""Stored blocks on the GPU (include/rcx_stored.h): the mix behind the block encode call against stored.mix_numpy, exactly;
the decode of any picks of a mixed set against the source and against the item call on the unmixed set; what both refuse
and latch; the host-buffer calls; and the version-3 containers that pack(..., stored=...) and pack_typed(..., stored=...) write.

The copy kernel (csrc/rcx_stored.hpp) gives an entry of at most 1024 bytes to one wave, four to a workgroup, and a longer one
to the whole workgroup; a fixed grid loops.  The shapes of stored_cases cover both kinds of entry and their border (1024,
1040), blocks off the 16-byte pieces (100), a ragged last block and one of a single byte, every pairing of source and
destination misalignment, and grids that loop.  The streams are the GPU encoders' own, which other tests hold to the oracle.
"""
import numpy as np
import pytest

import stored_cases as sc
from cpprcoder_amd import container, rcx, stored
from gpu_support import Guarded, ctx, decode_items, gpu_encode  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_STREAMS = {}


def streams(ctx, name, block, coder, tail=None):
    """(the bytes, the GPU encoder's payload, its offsets) of a fixture, made once."""
    key = (name, block, coder, tail)
    if key not in _STREAMS:
        n = (sc.NBLOCKS - 1) * block + (block - 7 if tail is None else tail)
        x = {"mixed": lambda: sc.mixed_bytes(block, tail), "shrinking": lambda: sc.shrinking_bytes(n), "fp32": lambda: sc.fp32_planes(block)}[name]()
        payload, offsets, _ = gpu_encode(ctx, x, block, coder=coder)
        _STREAMS[key] = (x, payload, offsets)
    return _STREAMS[key]


def table(offsets, salt):
    t = np.ascontiguousarray(np.asarray(offsets).astype(np.int64))
    return Guarded(8 * len(t), 0, t.view(np.uint8), salt=salt)


class Mix:
    """One call of the device mix with every buffer guarded; `cap` = the destination's size (n if None)."""

    def __init__(self, ctx, x, block, payload, offsets, gain, src_offset=0, comp_offset=0, dst_offset=0, cap=None, call=True):
        self.n, self.block, self.nblocks = len(x), block, rcx.block_count(len(x), block)
        self.src = Guarded(len(x), src_offset, x, salt=1)
        self.comp = Guarded(len(payload), comp_offset, payload, salt=4)
        self.offs_in = table(offsets, 5)
        self.dst = Guarded(len(x) if cap is None else cap, dst_offset, salt=2)
        self.offs_out = Guarded(8 * (self.nblocks + 1), 0, salt=3)
        self.flags = Guarded(self.nblocks, 0, salt=7)
        assert self.src.view.data_ptr() % 16 == src_offset % 16 and self.dst.view.data_ptr() % 16 == dst_offset % 16
        if call:
            self.run(ctx, gain)

    def run(self, ctx, gain):
        stored.mix_device(ctx, self.src.view, self.block, self.comp.view, self.comp.size, self.offs_in.view.view(torch.int64), gain, self.dst.view,
                          self.offs_out.view.view(torch.int64), self.flags.view)

    def read(self, ctx, label):
        """-> (mixed payload, offsets, flags, status, first bad block) after checking that nothing else was written."""
        st, bad = ctx.sync_status(raise_on_error=False)
        moffs = self.offs_out.view.view(torch.int64).cpu().numpy().astype(np.uint64)
        for g, written, what in ((self.src, 0, "src"), (self.comp, 0, "comp"), (self.offs_in, 0, "comp_offsets"), (self.offs_out, 8 * (self.nblocks + 1), "offsets"),
                                 (self.flags, self.nblocks, "stored"), (self.dst, min(int(moffs[-1]), self.dst.size), "dst")):
            g.check(written, f"{label}: {what}")
        return self.dst.view[: min(int(moffs[-1]), self.dst.size)].cpu().numpy(), moffs, self.flags.view.cpu().numpy(), st, bad

    def untouched(self, label):
        for g, what in ((self.src, "src"), (self.comp, "comp"), (self.offs_in, "comp_offsets"), (self.offs_out, "offsets"), (self.flags, "stored"), (self.dst, "dst")):
            g.check(0, f"{label}: {what}")


def assert_mix(ctx, x, block, payload, offsets, gain, label, **where):
    want = stored.mix_numpy(x, block, payload, offsets, gain)
    mixed, moffs, flags, st, _ = Mix(ctx, x, block, payload, offsets, gain, **where).read(ctx, label)
    assert st == rcx.OK, (label, st)
    assert np.array_equal(flags, want[2]), (label, "flags", flags, want[2])
    assert np.array_equal(moffs, want[1]), (label, "offsets")
    assert np.array_equal(mixed, want[0]), (label, "payload")
    return mixed, moffs, flags


# ---- mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", sc.CODERS)
def test_mix_against_numpy(ctx, coder):
    k = 0
    for block in sc.BLOCKS:
        for tail in (None, 1):
            x, payload, offsets = streams(ctx, "mixed", block, coder, tail)
            for gain in sc.GAINS:
                where = dict(src_offset=sc.OFFSETS[k % 5], dst_offset=sc.OFFSETS[(k // 5 + k) % 5], comp_offset=sc.OFFSETS[(k // 3) % 5])
                k += 1
                _, moffs, flags = assert_mix(ctx, x, block, payload, offsets, gain, (coder, block, tail, gain, where), **where)
                assert int(moffs[-1]) <= len(x)
                if gain == 65535:
                    assert bool(flags.all())


def test_every_pairing_of_misalignments(ctx):
    """Adaptive streams at 1040 (workgroup entries, both kinds of block) and 100 (wave entries): source and destination at
    every pair of the five offsets."""
    for block in (1040, 100):
        x, payload, offsets = streams(ctx, "mixed", block, 0)
        assert 0 < int(stored.mix_numpy(x, block, payload, offsets, 0)[2].sum()) < sc.NBLOCKS
        for s in sc.OFFSETS:
            for d in sc.OFFSETS:
                assert_mix(ctx, x, block, payload, offsets, 0, (block, s, d), src_offset=s, dst_offset=d, comp_offset=(s + 2 * d) % 16)


@pytest.mark.parametrize("coder", sc.CODERS)
def test_nothing_stored_is_the_input(ctx, coder):
    for block in (4096, 65536):
        x, payload, offsets = streams(ctx, "shrinking", block, coder)
        mixed, moffs, flags = assert_mix(ctx, x, block, payload, offsets, 0, (coder, block), src_offset=1, dst_offset=3)
        assert not flags.any() and np.array_equal(moffs, offsets) and np.array_equal(mixed, payload)


def test_fp32_planes(ctx):
    y, payload, offsets = streams(ctx, "fp32", 65536, 0, 65536)
    y = y[: 4 * 65536]
    assert len(offsets) == 5
    assert assert_mix(ctx, y, 65536, payload, offsets, 0, "fp32 gain 0")[2].tolist() == [1, 1, 0, 0]
    assert assert_mix(ctx, y, 65536, payload, offsets, 256, "fp32 gain 256", dst_offset=8)[2].tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("count", (65535, 65536, 65537))
def test_grids_that_loop(ctx, count):
    """Blocks of 16 bytes: more work units than the copy kernel's grid has workgroups, more blocks than a thread of the scan
    takes alone.  The mix reads the table and copies, it does not look into a stream: the streams here are random bytes of
    1 .. 24 bytes each, so that both kinds of block occur."""
    rs = np.random.RandomState(count)
    n = count * 16 - 5
    x = rs.randint(0, 256, n).astype(np.uint8)
    sizes = rs.randint(1, 25, count)
    offsets = np.zeros(count + 1, np.uint64)
    np.cumsum(sizes, out=offsets[1:])
    payload = rs.randint(0, 256, int(offsets[-1])).astype(np.uint8)
    _, _, flags = assert_mix(ctx, x, 16, payload, offsets, 0, count, src_offset=3, dst_offset=1, comp_offset=15)
    assert 0 < int(flags.sum()) < count


def test_a_captured_mix_replays(ctx):
    """Three launches in a row, no branches; captured once and replayed on two sets of streams."""
    block = 4096
    first = streams(ctx, "mixed", block, 0)
    second = (sc.mixed_bytes(block, seed=8),)
    second += gpu_encode(ctx, second[0], block, coder=0)[:2]
    room = max(len(first[1]), len(second[1]))
    d_src = torch.zeros(len(first[0]), dtype=torch.uint8, device="cuda")
    d_comp = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(sc.NBLOCKS + 1, dtype=torch.int64, device="cuda")
    dst = Guarded(len(first[0]), 3, salt=2)
    d_moffs = torch.zeros(sc.NBLOCKS + 1, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(sc.NBLOCKS, dtype=torch.uint8, device="cuda")

    def load(x, payload, offsets):
        d_src.copy_(torch.from_numpy(x.copy()))
        d_comp[: len(payload)].copy_(torch.from_numpy(payload.copy()))
        d_offs.copy_(torch.from_numpy(offsets.astype(np.int64)))

    def call():
        stored.mix_device(ctx, d_src, block, d_comp, room, d_offs, 0, dst.view, d_moffs, d_flags)

    load(*first)
    call()  # once outside, so that nothing happens for the first time in the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for x, payload, offsets in (second, first):
        load(x, payload, offsets)
        d_moffs.zero_()
        d_flags.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = stored.mix_numpy(x, block, payload, offsets, 0)
        assert np.array_equal(d_flags.cpu().numpy(), want[2]) and np.array_equal(d_moffs.cpu().numpy().astype(np.uint64), want[1])
        assert np.array_equal(dst.view[: len(want[0])].cpu().numpy(), want[0])
    dst.check(len(first[0]), "dst")
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK


# ---- decode ------------------------------------------------------------------------------------------------------------------
def decode_on_gpu(ctx, payload, offsets, flags, lengths, coder, pick=None, comp_offset=0, dst_offset=0):
    """stored.decode_device, guarded -> (list of the picks' bytes, status, first bad position, the output buffer).  `lengths`:
    the decoded length of every stream of the set."""
    comp = Guarded(len(payload), comp_offset, payload, salt=4)
    offs = table(offsets, 5)
    lengths = np.asarray(lengths, dtype=np.uint64)
    picked = lengths if pick is None else lengths[np.asarray(pick, dtype=np.int64)]
    doffs = rcx.item_offsets(picked)
    out = Guarded(int(doffs[-1]), dst_offset, salt=6)
    stored.decode_device(ctx, comp.view, len(payload), offs.view.view(torch.int64), flags, doffs, out.view, pick=pick, coder=coder)
    st, bad = ctx.sync_status(raise_on_error=False)
    comp.check(0, "decode comp")
    offs.check(0, "decode table")
    out.check(int(doffs[-1]), "decode dst")
    flat = out.view.cpu().numpy()
    return [flat[int(doffs[k]): int(doffs[k + 1])] for k in range(len(picked))], st, bad, out


DECODE_CASES = ((0, 100), (0, 1040), (1, 1024), (0, 4096), (1, 4096), (2, 4096), (0, 65536), (1, 65536), (2, 65536), (3, 65536))


@pytest.mark.parametrize("coder,block", DECODE_CASES)
def test_decode_any_picks(ctx, coder, block):
    x, payload, offsets = streams(ctx, "mixed", block, coder)
    mixed, moffs, flags = stored.mix_numpy(x, block, payload, offsets, 0)
    lengths = stored.block_lengths(len(x), block)
    blocks = [x[b * block: b * block + int(lengths[b])] for b in range(sc.NBLOCKS)]
    raw, kept = np.flatnonzero(flags), np.flatnonzero(flags == 0)
    assert len(raw) and len(kept), "both kinds of stream"
    picks = {"all": None, "repeated": [1, 5, 1, 0, 0, 5, 5], "unordered": [5, 2, 0, 4, 1, 3], "a subset": [4, 1], "only stored": list(raw[::-1]),
             "only kept": list(kept), "empty": []}
    for k, (name, pick) in enumerate(picks.items()):
        where = dict(comp_offset=sc.OFFSETS[k % 5], dst_offset=sc.OFFSETS[(k + 2) % 5])
        got, st, _, _ = decode_on_gpu(ctx, mixed, moffs, flags, lengths, coder, pick, **where)
        assert st == rcx.OK, (name, st)
        order = range(sc.NBLOCKS) if pick is None else pick
        assert len(got) == len(order)
        for j, b in enumerate(order):
            assert np.array_equal(got[j], blocks[b]), (name, "position", j, "block", b)
        # and what the item call makes of the same picks of the unmixed set
        same, st, _ = decode_items(ctx, payload, offsets, [int(lengths[b]) for b in order], coder, pick=pick, **where)
        assert st == rcx.OK and all(np.array_equal(a, b) for a, b in zip(got, same)), name


def test_without_the_table_it_is_the_item_call(ctx):
    x, payload, offsets = streams(ctx, "mixed", 4096, 0)
    lengths = stored.block_lengths(len(x), 4096)
    pick = [3, 1, 5, 1]
    want, st, _ = decode_items(ctx, payload, offsets, [int(lengths[b]) for b in pick], 0, pick=pick, dst_offset=3)
    assert st == rcx.OK
    for flags in (None, np.zeros(sc.NBLOCKS, np.uint8)):
        got, st, _, _ = decode_on_gpu(ctx, payload, offsets, flags, lengths, 0, pick, dst_offset=3)
        assert st == rcx.OK and all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- failures ----------------------------------------------------------------------------------------------------------------
def resized(mixed, moffs, b, by):
    """The mixed set with stream b `by` bytes longer (one byte put behind it) or shorter."""
    parts = [mixed[int(moffs[i]): int(moffs[i + 1])] for i in range(len(moffs) - 1)]
    parts[b] = np.concatenate([parts[b], np.full(by, 0x5A, np.uint8)]) if by > 0 else parts[b][:by]
    offs = np.zeros(len(moffs), np.uint64)
    np.cumsum([len(p) for p in parts], out=offs[1:])
    return np.concatenate(parts), offs


@pytest.mark.parametrize("block", (100, 4096))
def test_a_stored_stream_of_the_wrong_length(ctx, block):
    x, payload, offsets = streams(ctx, "mixed", block, 0)
    mixed, moffs, flags = stored.mix_numpy(x, block, payload, offsets, 0)
    assert flags.tolist() == [1, 0, 1, 0, 1, 0]
    lengths = stored.block_lengths(len(x), block)
    pick = [5, 4, 1, 2, 0, 3, 2]  # stream 2 at positions 3 and 6
    for by in (-1, 1):
        bad_mixed, bad_offs = resized(mixed, moffs, 2, by)
        got, st, first, out = decode_on_gpu(ctx, bad_mixed, bad_offs, flags, lengths, 0, pick, dst_offset=1)
        assert (st, first) == (rcx.E_CORRUPT, 3), (by, st, first)
        doffs = rcx.item_offsets(lengths[pick])
        for j, b in enumerate(pick):
            if b == 2:  # nothing of that entry was written
                lo, hi = out.at + int(doffs[j]), out.at + int(doffs[j + 1])
                assert torch.equal(out.tensor[lo:hi], out.before[lo:hi]), (by, j)
            else:
                assert np.array_equal(got[j], x[b * block: b * block + int(lengths[b])]), (by, j, b)
    # a kept stream later in the call is damaged too (cut to 3 bytes: below any stream's frame): the lowest position wins
    parts_mixed, parts_offs = resized(mixed, moffs, 2, -1)
    cut = int(parts_offs[4] - parts_offs[3]) - 3
    both_mixed, both_offs = resized(parts_mixed, parts_offs, 3, -cut)
    for pick, want in (([0, 2, 1, 3, 5], 1), ([0, 3, 1, 2, 5], 1), ([3, 2], 0), ([2, 3], 0), ([1, 5, 4, 3], 3)):
        got, st, first, _ = decode_on_gpu(ctx, both_mixed, both_offs, flags, lengths, 0, pick)
        assert (st, first) == (rcx.E_CORRUPT, want), (pick, st, first)
        for j, b in enumerate(pick):
            if b not in (2, 3):
                assert np.array_equal(got[j], x[b * block: b * block + int(lengths[b])]), (pick, j)
    # offsets that leave the buffer or go backwards: not followed
    for damage in (lambda o: o.__setitem__(3, o[3] + np.uint64(1 << 40)), lambda o: o.__setitem__(2, o[3] + np.uint64(1))):
        offs = moffs.copy()
        damage(offs)
        _, st, first, _ = decode_on_gpu(ctx, mixed, offs, flags, lengths, 0, [0, 2, 4])
        assert (st, first) == (rcx.E_CORRUPT, 1)
    assert decode_on_gpu(ctx, mixed, moffs, flags, lengths, 0, pick)[1] == rcx.OK  # the latch is clear again


def test_mix_capacity_and_a_bad_table(ctx):
    x, payload, offsets = streams(ctx, "mixed", 4096, 0)
    want = stored.mix_numpy(x, 4096, payload, offsets, 0)
    total = int(want[1][-1])
    m = Mix(ctx, x, 4096, payload, offsets, 0, dst_offset=3, cap=total - 1)
    mixed, moffs, flags, st, bad = m.read(ctx, "one below the total")  # (read: nothing behind the cap was written)
    assert (st, bad) == (rcx.E_CAPACITY, sc.NBLOCKS) and int(moffs[-1]) == total and np.array_equal(flags, want[2])
    assert np.array_equal(mixed[: int(moffs[5])], want[0][: int(moffs[5])])  # every stream that fits is there
    mixed, _, _, st, _ = Mix(ctx, x, 4096, payload, offsets, 0, cap=total).read(ctx, "just enough")
    assert st == rcx.OK and np.array_equal(mixed, want[0])
    # an entry of the input table that points past comp_size, and one that decreases: not followed, latched at that block
    for at, value, first in ((4, np.uint64(len(payload) + 1), 3), (2, np.uint64(0), 1)):
        offs = offsets.copy()
        offs[at] = value
        _, moffs, _, st, bad = Mix(ctx, x, 4096, payload, offs, 0).read(ctx, "bad table")
        assert (st, bad) == (rcx.E_CORRUPT, first) and moffs[first + 1] == moffs[first]


def test_bad_arguments_write_nothing(ctx):
    x, payload, offsets = streams(ctx, "mixed", 4096, 0)
    m = Mix(ctx, x, 4096, payload, offsets, 0, call=False)
    L, h, n = stored.lib(), ctx._h, len(x)
    s = torch.cuda.current_stream().cuda_stream
    src, comp, offs_in, dst = m.src.view.data_ptr(), m.comp.view.data_ptr(), m.offs_in.view.data_ptr(), m.dst.view.data_ptr()
    offs_out, flags, size = m.offs_out.view.data_ptr(), m.flags.view.data_ptr(), len(payload)

    def mix(src=src, n=n, block=4096, comp=comp, size=size, offs_in=offs_in, gain=0, dst=dst, cap=n, offs_out=offs_out, flags=flags, handle=h):
        return L.rcx_stored_mix_device(handle, src, n, block, comp, size, offs_in, gain, dst, cap, offs_out, flags, s)

    refused = [mix(block=15), mix(block=0), mix(block=rcx.MAX_BLOCK + 1), mix(gain=65536), mix(gain=1 << 31), mix(handle=None),
               mix(src=None), mix(comp=None), mix(offs_in=None), mix(dst=None), mix(offs_out=None), mix(flags=None), mix(n=0, offs_out=None),
               mix(dst=src), mix(dst=src + n - 1), mix(dst=src - n + 1), mix(dst=comp), mix(dst=comp + size - 1), mix(dst=comp - n + 1)]
    assert refused == [rcx.E_ARG] * len(refused), refused
    torch.cuda.synchronize()
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    m.untouched("after the refusals")
    # n = 0 writes offsets[0] = 0 and nothing else, whatever the other pointers are
    assert mix(n=0, src=None, comp=None, offs_in=None, dst=None, flags=None, size=0, cap=0) == rcx.OK
    torch.cuda.synchronize()
    m.offs_out.check(8, "n = 0")
    assert int(m.offs_out.view.view(torch.int64)[0]) == 0
    m.dst.check(0, "n = 0")
    # decode: the item call's refusals, with a table that has a stored stream
    mixed, moffs, marks = stored.mix_numpy(x, 4096, payload, offsets, 0)
    d_comp, d_offs, out = Guarded(len(mixed), 0, mixed, salt=4), table(moffs, 5), Guarded(n, 0, salt=6)
    f = np.ascontiguousarray(marks)
    doffs = rcx.item_offsets(stored.block_lengths(n, 4096))
    down, long = np.array([0, 4096, 100], np.uint64), np.array([0, rcx.MAX_BLOCK + 1], np.uint64)
    past = np.array([6], np.uint64)

    def dec(handle=h, coder=0, comp=d_comp.view.data_ptr(), offs=d_offs.view.data_ptr(), nstreams=6, pick=None, npick=6, doffs=doffs.ctypes.data,
            dst=out.view.data_ptr()):
        return L.rcx_stored_decode_device(handle, coder, comp, len(mixed), offs, nstreams, f.ctypes.data, pick, npick, doffs, dst, s)

    refused = [dec(handle=None), dec(coder=4), dec(doffs=None), dec(comp=None), dec(offs=None), dec(dst=None), dec(doffs=down.ctypes.data, npick=2),
               dec(doffs=long.ctypes.data, npick=1), dec(pick=past.ctypes.data, npick=1)]
    assert refused == [rcx.E_ARG] * len(refused), refused
    assert dec(npick=0) == rcx.OK
    torch.cuda.synchronize()
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    out.check(0, "after the refusals")
    assert dec() == rcx.OK and ctx.sync_status(raise_on_error=False)[0] == rcx.OK  # and the context still works
    assert np.array_equal(out.view.cpu().numpy(), x)


# ---- the host-buffer calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder,block", ((0, 100), (1, 1040), (2, 4096), (3, 65536)))
def test_host_calls_equal_the_device_calls(ctx, coder, block):
    x, payload, offsets = streams(ctx, "mixed", block, coder)
    lengths = stored.block_lengths(len(x), block)
    for gain in (0, 256):
        want = stored.mix_numpy(x, block, payload, offsets, gain)
        mixed, moffs, flags = stored.mix(ctx, x, block, payload, offsets, gain)
        assert np.array_equal(mixed, want[0]) and np.array_equal(moffs, want[1]) and np.array_equal(flags, want[2])
        for pick in (None, [5, 0, 3, 3], []):
            got = stored.decode(ctx, mixed, moffs, flags, lengths, pick=pick, coder=coder)
            device = decode_on_gpu(ctx, mixed, moffs, flags, lengths, coder, pick)[0]
            assert len(got) == len(device) and all(np.array_equal(a, b) for a, b in zip(got, device))
            for j, b in enumerate(range(sc.NBLOCKS) if pick is None else pick):
                assert np.array_equal(got[j], x[b * block: b * block + int(lengths[b])])
    m, o, f = stored.mix(ctx, b"", 4096, b"", [0])
    assert len(m) == 0 and o.tolist() == [0] and len(f) == 0
    # a destination that is too small: the size comes back with the status
    size = rcx.C.c_uint64()
    small = np.zeros(16, np.uint8)
    src, comp, offs = np.ascontiguousarray(x), np.ascontiguousarray(payload), np.ascontiguousarray(offsets, dtype=np.uint64)
    st = stored.lib().rcx_stored_mix(ctx._h, src.ctypes.data, len(src), block, comp.ctypes.data, len(comp), offs.ctypes.data, 0, small.ctypes.data, 16,
                                     rcx.C.byref(size), None, None)
    assert st == rcx.E_CAPACITY and size.value == int(stored.mix_numpy(x, block, payload, offsets, 0)[1][-1]) and not small.any()


# ---- containers --------------------------------------------------------------------------------------------------------------
def flags_of(blob, typed=False):
    c = (container.parse_typed if typed else container.parse)(blob)
    return c, (np.zeros(c["nblocks"], bool) if c["stored"] is None else c["stored"])


@pytest.mark.parametrize("coder", sc.CODERS)
def test_pack_and_unpack(ctx, coder):
    block = 65536 if coder == 3 else 4096
    x, payload, offsets = streams(ctx, "mixed", block, coder)
    want = stored.mix_numpy(x, block, payload, offsets, 0)
    for checksum in (False, True):
        blob = container.pack(x, block, coder, ctx, checksum=checksum, stored=True)
        c, marks = flags_of(blob)
        assert blob[4] == 3 and c["flags"] == (6 if checksum else 4) and (c["crcs"] is not None) == checksum
        assert np.array_equal(marks, want[2] != 0) and np.array_equal(c["offsets"], want[1]) and np.array_equal(c["payload"], want[0])
        if checksum:  # the CRC of the bytes the coder saw, as without the option
            assert np.array_equal(c["crcs"], container.parse(container.pack(x, block, coder, ctx, checksum=True))["crcs"])
        assert container.unpack(blob, ctx) == x.tobytes() and container.unpack(blob, ctx, verify=False) == x.tobytes()
        for lo, hi in ((0, len(x)), (block - 3, 3 * block + 5), (2 * block, 2 * block + 1), (len(x) - 9, len(x)), (5 * block, 5 * block)):
            assert container.unpack_range(blob, lo, hi, ctx) == x[lo:hi].tobytes(), (checksum, lo, hi)
    # a fraction: more blocks stored, never fewer
    more = flags_of(container.pack(x, block, coder, ctx, stored=0.3))[1]
    assert bool((more >= (want[2] != 0)).all()) and np.array_equal(more, stored.mix_numpy(x, block, payload, offsets, stored.gain_q16(0.3))[2] != 0)


def test_pack_with_the_block_sort(ctx):
    x = sc.mixed_bytes(65536)
    for checksum in (False, True):
        blob = container.pack(x, 65536, 0, ctx, blksort=True, checksum=checksum, stored=True)
        c, marks = flags_of(blob)
        plain = container.parse(container.pack(x, 65536, 0, ctx, blksort=True, checksum=checksum))
        assert blob[4] == 3 and c["flags"] == (7 if checksum else 5) and c["nblocks"] == plain["nblocks"] == 7
        # the mix's source is what the coder saw: the block-sorted text
        sizes, lengths = np.diff(plain["offsets"].astype(np.int64)), stored.block_lengths(container.coded_size(len(x), 1), 65536)
        assert np.array_equal(marks, stored.is_stored(sizes, lengths, 0)) and marks.any() and not marks.all()
        assert len(c["payload"]) < len(plain["payload"]) and container.unpack(blob, ctx) == x.tobytes()
        with pytest.raises(container.ContainerError):
            container.unpack_range(blob, 0, 10, ctx)


@pytest.mark.parametrize("predict", (None, "delta", "zigzag"))
def test_pack_typed(ctx, predict):
    x = sc.fp32_bytes()
    for coder, gain_arg, want in ((0, True, [1, 1, 0, 0]), (0, 256 / 65536, [1, 1, 1, 0]), (3, True, [1, 1, 1, 0])):
        for checksum in (False, True):
            blob = container.pack_typed(x, 4, 65536, coder, ctx, checksum=checksum, predict=predict, stored=gain_arg)
            today = container.pack_typed(x, 4, 65536, coder, ctx, checksum=checksum, predict=predict)
            c, marks = flags_of(blob, typed=True)
            assert blob[4] == 3 and blob[29] == container.PREDICTORS[predict] and c["flags"] == (6 if checksum else 4)
            if predict is None:
                assert marks.tolist() == [bool(v) for v in want], (coder, gain_arg, marks)
            t = container.parse_typed(today)
            sizes = np.diff(t["offsets"].astype(np.int64))
            assert np.array_equal(marks, stored.is_stored(sizes, np.full(4, 65536), stored.gain_q16(gain_arg)))  # the source is the predicted, split text
            assert len(c["payload"]) <= len(x) and len(blob) < len(today)
            if checksum:
                assert np.array_equal(c["crcs"], t["crcs"])
            assert container.unpack_typed(blob, ctx) == x.tobytes()
            for lo, hi in ((0, len(x)), (7, 9), (len(x) - 5, len(x))):
                assert container.unpack_typed_range(blob, lo, hi, ctx) == x[lo:hi].tobytes()


def test_pack_typed_on_several_superblocks_and_a_gpu_tensor(ctx):
    x = sc.fp32_bytes(5 * 4 * 4096 + 1236)  # five superblocks and a ragged sixth
    t = torch.from_numpy(x.copy()).cuda().view(torch.float32)
    blob = container.pack_typed(t, None, 4096, 1, ctx, checksum=True, stored=True)
    assert blob == container.pack_typed(x, 4, 4096, 1, ctx, checksum=True, stored=True) and blob[4] == 3
    c, marks = flags_of(blob, typed=True)
    assert marks[0] and marks[1] and marks[4] and marks[5] and not marks.all() and len(c["payload"]) <= len(x)
    assert container.unpack_typed(blob, ctx) == x.tobytes()
    lo, hi = 4 * 4096 - 5, 3 * 4 * 4096 + 77
    assert container.unpack_typed_range(blob, lo, hi, ctx) == x[lo:hi].tobytes()
    assert container.unpack_typed_range(blob, len(x) - 100, len(x), ctx) == x[-100:].tobytes()


def test_a_flipped_byte_in_a_stored_block(ctx):
    x, _, _ = streams(ctx, "mixed", 4096, 0)
    for checksum in (True, False):
        blob = bytearray(container.pack(x, 4096, 0, ctx, checksum=checksum, stored=True))
        c, marks = flags_of(bytes(blob))
        assert marks[2]
        at = len(blob) - len(c["payload"]) + int(c["offsets"][2]) + 1000
        blob[at] ^= 0x10
        if checksum:
            for call in (lambda: container.unpack(bytes(blob), ctx), lambda: container.unpack_range(bytes(blob), 2 * 4096 + 5, 2 * 4096 + 9, ctx)):
                with pytest.raises(container.ChecksumError) as e:
                    call()
                assert e.value.index == 2 and e.value.kind == "block"
            assert container.unpack_range(bytes(blob), 0, 2 * 4096, ctx) == x[: 2 * 4096].tobytes()  # the blocks in front verify
        back = np.frombuffer(container.unpack(bytes(blob), ctx, verify=False), np.uint8)
        assert np.flatnonzero(back != x).tolist() == [2 * 4096 + 1000] and back[2 * 4096 + 1000] == x[2 * 4096 + 1000] ^ 0x10
    typed = bytearray(container.pack_typed(sc.fp32_bytes(), 4, 65536, 0, ctx, checksum=True, stored=True))
    c, _ = flags_of(bytes(typed), typed=True)
    typed[len(typed) - len(c["payload"]) + int(c["offsets"][1]) + 77] ^= 1
    with pytest.raises(container.ChecksumError) as e:
        container.unpack_typed(bytes(typed), ctx)
    assert e.value.index == 1


def test_nothing_stored_is_todays_container(ctx):
    x = sc.shrinking_bytes(6 * 4096 - 7)
    for coder in sc.CODERS:
        for checksum in (False, True):
            today = container.pack(x, 4096, coder, ctx, checksum=checksum)
            assert container.pack(x, 4096, coder, ctx, checksum=checksum, stored=True) == today and today[4] == (2 if checksum else 1)
    steps = np.arange(5 * 4096, dtype=np.int32) // 1024  # every plane of it, and of its differences, shrinks
    for predict in (None, "delta"):
        for checksum in (False, True):
            today = container.pack_typed(steps, None, 4096, 0, ctx, checksum=checksum, predict=predict)
            assert container.pack_typed(steps, None, 4096, 0, ctx, checksum=checksum, predict=predict, stored=True) == today
            assert today[4] == (2 if predict else 1) and container.unpack_typed(today, ctx) == steps.tobytes()


@pytest.mark.parametrize("coder", sc.CODERS)
def test_uniform_input_never_grows(ctx, coder):
    for block in (4096, 65536):
        x = np.random.RandomState(block + coder).randint(0, 256, 5 * block + 99).astype(np.uint8)
        blob, today = container.pack(x, block, coder, ctx, stored=True), container.pack(x, block, coder, ctx)
        c, marks = flags_of(blob)
        print(coder, block, len(today), len(blob), len(x))
        assert len(c["payload"]) <= len(x) and len(blob) < len(today) and bool(marks[:5].all())
        assert container.unpack(blob, ctx) == x.tobytes()


def test_the_command_line_says_how_many(ctx, tmp_path, capsys):
    from cpprcoder_amd.__main__ import main
    x = sc.mixed_bytes(4096)
    (tmp_path / "mixed.bin").write_bytes(x.tobytes())
    assert main(["t", "-b", "4096", "--stored", "--crc", str(tmp_path / "mixed.bin")]) == 0
    out = capsys.readouterr().out
    rows = [line for line in out.splitlines() if ".bin|" in line]
    assert len(rows) == 1 and rows[0].endswith(" stored 3/6") and "MISMATCH" not in out, out
    assert main(["c", "--planes", "4", "--stored=0.004", "--predict", "auto", str(tmp_path / "mixed.bin"), str(tmp_path / "mixed.rcxt")]) == 0
    line = capsys.readouterr().out.strip()
    assert " stored " in line and " predict=" in line and line.index(" stored ") < line.index(" predict="), line
    assert main(["d", str(tmp_path / "mixed.rcxt"), str(tmp_path / "back.bin")]) == 0
    assert (tmp_path / "back.bin").read_bytes() == x.tobytes()
