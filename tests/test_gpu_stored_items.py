"""Stored items on the GPU (include/rcx_stored_items.h): the mix behind the item encode call against
stored_items.mix_items_numpy, exactly; what it refuses and latches; the host-buffer call; the round trip through
stored.decode_device; and the RCXJ version-2 containers that pack_typed_items(..., stored=...) and pack_tensors(..., stored=...) write.

The copy kernel gives an entry of at most 1024 bytes to one wave, four to a workgroup, and a longer one to the whole workgroup,
whose unrolled loop begins at 12 288 bytes; unlike the block mix a call has entries of both kinds, stored and kept, planned
longest first.  The batch of stored_items_cases.LENGTHS has every border and two empty items; its contents rotate so that every
length is uniform, Zipf and one repeated byte in turn.  The streams are the GPU encoders' own, which other tests hold to the
oracle.  Every buffer lies between guard bytes.
"""
import numpy as np
import pytest

import stored_cases as sc
import stored_items_cases as sic
from cpprcoder_amd import container, rcx, stored, stored_items
from gpu_support import Guarded, ctx, encode_items  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_STREAMS = {}


def streams(ctx, coder, first_kind=0):
    """(the items, the GPU encoder's payload, its offsets) of the batch, made once."""
    key = (coder, first_kind)
    if key not in _STREAMS:
        items = sic.batch(sic.LENGTHS, first_kind)
        _STREAMS[key] = (items,) + tuple(encode_items(ctx, items, coder))
    return _STREAMS[key]


def table(offsets, salt):
    t = np.ascontiguousarray(np.asarray(offsets).astype(np.int64))
    return Guarded(8 * len(t), 0, t.view(np.uint8), salt=salt)


class MixItems:
    """One call of the device mix with every buffer guarded; the items lie `base` bytes into the source; `cap` = the
    destination's size (the items' bytes if None)."""

    def __init__(self, ctx, items, payload, offsets, gain, src_offset=0, comp_offset=0, dst_offset=0, cap=None, base=0, call=True):
        self.nitems = len(items)
        self.soffs = sic.offsets_of([len(x) for x in items], base)
        self.x = np.concatenate([np.full(base, 0xEE, np.uint8)] + list(items)) if len(items) or base else np.zeros(0, np.uint8)
        n = len(self.x) - base
        self.src = Guarded(len(self.x), src_offset, self.x, salt=1)
        self.comp = Guarded(len(payload), comp_offset, payload, salt=4)
        self.offs_in = table(offsets, 5)
        self.dst = Guarded(n if cap is None else cap, dst_offset, salt=2)
        self.offs_out = Guarded(8 * (self.nitems + 1), 0, salt=3)
        self.flags = Guarded(self.nitems, 0, salt=7)
        assert len(self.x) == 0 or self.src.view.data_ptr() % 16 == src_offset % 16
        if call:
            stored_items.mix_items_device(ctx, self.src.view, self.soffs, self.comp.view, self.comp.size, self.offs_in.view.view(torch.int64), gain,
                                          self.dst.view, self.offs_out.view.view(torch.int64), self.flags.view)

    def read(self, ctx, label):
        """-> (mixed payload, offsets, flags, status, first bad item) after checking that nothing else was written."""
        st, bad = ctx.sync_status(raise_on_error=False)
        moffs = self.offs_out.view.view(torch.int64).cpu().numpy().astype(np.uint64)
        written = min(int(moffs[-1]), self.dst.size)
        for g, count, what in ((self.src, 0, "src"), (self.comp, 0, "comp"), (self.offs_in, 0, "comp_offsets"), (self.offs_out, 8 * (self.nitems + 1), "offsets"),
                               (self.flags, self.nitems, "stored"), (self.dst, written, "dst")):
            g.check(count, f"{label}: {what}")
        return self.dst.view[:written].cpu().numpy(), moffs, self.flags.view.cpu().numpy(), st, bad

    def untouched(self, label):
        for g, what in ((self.src, "src"), (self.comp, "comp"), (self.offs_in, "comp_offsets"), (self.offs_out, "offsets"), (self.flags, "stored"), (self.dst, "dst")):
            g.check(0, f"{label}: {what}")


def assert_mix(ctx, items, payload, offsets, gain, label, **where):
    m = MixItems(ctx, items, payload, offsets, gain, **where)
    want = stored_items.mix_items_numpy(m.x, m.soffs, payload, offsets, gain)
    mixed, moffs, flags, st, _ = m.read(ctx, label)
    assert st == rcx.OK, (label, st)
    assert np.array_equal(flags, want[2]), (label, "flags", flags, want[2])
    assert np.array_equal(moffs, want[1]), (label, "offsets")
    assert np.array_equal(mixed, want[0]), (label, "payload")
    return mixed, moffs, flags


# ---- mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", sic.CODERS)
def test_mix_against_numpy(ctx, coder):
    k = 0
    seen = set()
    for first_kind in (0, 1, 2):
        items, payload, offsets = streams(ctx, coder, first_kind)
        for gain in sic.GAINS:
            where = dict(src_offset=sic.OFFSETS[k % 5], dst_offset=sic.OFFSETS[(k // 5 + k) % 5], comp_offset=sic.OFFSETS[(k // 3) % 5], base=(0, 5)[k % 2])
            k += 1
            _, moffs, flags = assert_mix(ctx, items, payload, offsets, gain, (coder, first_kind, gain, where), **where)
            assert int(moffs[-1]) <= sum(sic.LENGTHS) and flags[0] == 0 and flags[14] == 0  # an empty item is never stored
            if gain == 65535:
                assert flags.tolist() == [int(n > 0) for n in sic.LENGTHS]
            if gain == 0:
                seen |= {(bool(f), n > sic.COPY_SHORT) for f, n in zip(flags, sic.LENGTHS) if n}
    # stored and kept entries of both kinds in one call; rANS keeps no item of 1024 bytes or less (its table alone has 1032)
    assert seen == {(True, True), (True, False), (False, True)} | ({(False, False)} if coder < 2 else set()), seen


def test_every_pairing_of_misalignments(ctx):
    items, payload, offsets = streams(ctx, 0, 0)
    for s in sic.OFFSETS:
        for d in sic.OFFSETS:
            assert_mix(ctx, items, payload, offsets, 0, (s, d), src_offset=s, dst_offset=d, comp_offset=(s + 2 * d + 1) % 16)


def random_streams(rs, lengths, spread):
    """The mix reads the table and copies, it does not look into a stream: random bytes, each stream within `spread` of its
    item's length, so that both kinds of item occur."""
    sizes = np.maximum(1, np.asarray(lengths, dtype=np.int64) + rs.randint(-spread, spread + 1, len(lengths)))
    offsets = sic.offsets_of(sizes)
    return rs.randint(0, 256, int(offsets[-1])).astype(np.uint8), offsets


@pytest.mark.parametrize("count", (65535, 65536, 65537))
def test_grids_that_loop(ctx, count):
    """Items of 16 bytes: more items than the size kernel's grid has threads at eight workgroups a CU, more work units than the
    copy kernel's grid has workgroups, more items than a thread of the scan takes alone."""
    rs = np.random.RandomState(count)
    x = rs.randint(0, 256, count * 16).astype(np.uint8)
    items = list(x.reshape(count, 16))
    payload, offsets = random_streams(rs, [16] * count, 8)
    _, _, flags = assert_mix(ctx, items, payload, offsets, 0, count, src_offset=3, dst_offset=1, comp_offset=15)
    assert 0 < int(flags.sum()) < count


def test_more_long_entries_than_workgroups(ctx):
    """Items of 1040 bytes, 37 more than the copy grid's eight workgroups a compute unit: the unit loop goes round."""
    count = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    rs = np.random.RandomState(37)
    items = list(rs.randint(0, 256, count * 1040).astype(np.uint8).reshape(count, 1040))
    payload, offsets = random_streams(rs, [1040] * count, 30)
    _, _, flags = assert_mix(ctx, items, payload, offsets, 0, "unit loop", src_offset=1, dst_offset=8, comp_offset=3)
    assert 0 < int(flags.sum()) < count


def test_only_empty_items_and_none(ctx):
    empty = [np.zeros(0, np.uint8)] * 5
    mixed, moffs, flags = assert_mix(ctx, empty, np.zeros(0, np.uint8), np.zeros(6, np.uint64), 65535, "only empty")
    assert len(mixed) == 0 and moffs.tolist() == [0] * 6 and flags.tolist() == [0] * 5
    mixed, moffs, flags = assert_mix(ctx, [], np.zeros(0, np.uint8), np.zeros(1, np.uint64), 0, "no items")
    assert len(mixed) == 0 and moffs.tolist() == [0] and len(flags) == 0
    # the zero table whatever the other pointers are
    t = Guarded(8 * 4, 0, salt=3)
    f = Guarded(3, 0, salt=7)
    soffs = np.array([7, 7, 7, 7], np.uint64)
    st = stored_items.lib().rcx_stored_mix_items_device(ctx._h, None, soffs.ctypes.data, 3, None, 0, None, 0, None, 0, t.view.data_ptr(), f.view.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream)
    assert st == rcx.OK and ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    t.check(32, "zero table")
    f.check(3, "zero flags")
    assert not t.view.any() and not f.view.any()


# ---- failures ----------------------------------------------------------------------------------------------------------------
def test_capacity_and_a_bad_table(ctx):
    items, payload, offsets = streams(ctx, 0, 0)
    x, soffs = np.concatenate(items), sic.offsets_of(sic.LENGTHS)
    want = stored_items.mix_items_numpy(x, soffs, payload, offsets, 0)
    total, nitems = int(want[1][-1]), len(items)
    m = MixItems(ctx, items, payload, offsets, 0, dst_offset=3, cap=total - 1)
    mixed, moffs, flags, st, bad = m.read(ctx, "one below the total")  # (read: nothing behind the cap was written)
    assert (st, bad) == (rcx.E_CAPACITY, nitems) and int(moffs[-1]) == total and np.array_equal(flags, want[2]) and np.array_equal(moffs, want[1])
    last = max(i for i in range(nitems) if moffs[i + 1] < total)  # every stream that ends inside the cap is there
    assert np.array_equal(mixed[: int(moffs[last + 1])], want[0][: int(moffs[last + 1])])
    mixed, _, _, st, _ = MixItems(ctx, items, payload, offsets, 0, cap=total).read(ctx, "just enough")
    assert st == rcx.OK and np.array_equal(mixed, want[0])
    # an entry of the input table that decreases, and one that points past comp_size: not followed, latched at that item,
    # whose stream is empty and whose flag is 0; every other item is right
    for at, value, first in ((10, offsets[9] - np.uint64(1), 9), (6, np.uint64(len(payload) + 1), 5)):
        offs = offsets.copy()
        offs[at] = value
        mixed, moffs, flags, st, bad = MixItems(ctx, items, payload, offs, 0, src_offset=1).read(ctx, "bad table")
        assert (st, bad) == (rcx.E_CORRUPT, first) and moffs[first + 1] == moffs[first] and flags[first] == 0
        for i in range(nitems):
            if i in (first, at):  # (the entry behind the damaged one is read through it)
                continue
            got = mixed[int(moffs[i]): int(moffs[i + 1])]
            assert flags[i] == want[2][i] and np.array_equal(got, want[0][int(want[1][i]): int(want[1][i + 1])]), (at, i)
    assert MixItems(ctx, items, payload, offsets, 0).read(ctx, "again")[3] == rcx.OK  # the latch is clear again


def test_bad_arguments_write_nothing(ctx):
    items, payload, offsets = streams(ctx, 0, 0)
    m = MixItems(ctx, items, payload, offsets, 0, call=False)
    L, h, n, nitems = stored_items.lib(), ctx._h, len(m.x), len(items)
    s = torch.cuda.current_stream().cuda_stream
    src, comp, offs_in, dst = m.src.view.data_ptr(), m.comp.view.data_ptr(), m.offs_in.view.data_ptr(), m.dst.view.data_ptr()
    offs_out, flags, size = m.offs_out.view.data_ptr(), m.flags.view.data_ptr(), len(payload)
    good = m.soffs
    down, long = good.copy(), np.array([0, rcx.MAX_BLOCK + 1], np.uint64)
    down[4] = down[3] - np.uint64(1)

    def mix(src=src, soffs=good, nitems=nitems, comp=comp, size=size, offs_in=offs_in, gain=0, dst=dst, cap=n, offs_out=offs_out, flags=flags, handle=h):
        return L.rcx_stored_mix_items_device(handle, src, None if soffs is None else soffs.ctypes.data, nitems, comp, size, offs_in, gain, dst, cap, offs_out,
                                             flags, s)

    refused = [mix(soffs=down), mix(soffs=long, nitems=1), mix(gain=65536), mix(gain=1 << 31), mix(nitems=0x80000000), mix(handle=None),
               mix(src=None), mix(soffs=None), mix(comp=None), mix(offs_in=None), mix(dst=None), mix(offs_out=None), mix(flags=None),
               mix(nitems=0, offs_out=None),
               mix(dst=src), mix(dst=src + n - 1), mix(dst=src - n + 1), mix(dst=comp), mix(dst=comp + size - 1), mix(dst=comp - n + 1)]
    assert refused == [rcx.E_ARG] * len(refused), refused
    torch.cuda.synchronize()
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    m.untouched("after the refusals")
    # the host-buffer call's refusals
    x, pay = np.ascontiguousarray(m.x), np.ascontiguousarray(payload)
    offs, out, total = np.ascontiguousarray(offsets, dtype=np.uint64), np.zeros(n, np.uint8), rcx.C.c_uint64(77)

    def host(src=x.ctypes.data, soffs=good, nitems=nitems, comp=pay.ctypes.data, offs=offs.ctypes.data, gain=0, dst=out.ctypes.data, total=rcx.C.byref(total),
             handle=h):
        return L.rcx_stored_mix_items(handle, src, None if soffs is None else soffs.ctypes.data, nitems, comp, len(pay), offs, gain, dst, n, total, None, None)

    refused = [host(soffs=down), host(soffs=long, nitems=1), host(gain=65536), host(nitems=0x80000000), host(handle=None), host(src=None), host(soffs=None),
               host(comp=None), host(offs=None), host(dst=None), host(total=None)]
    assert refused == [rcx.E_ARG] * len(refused) and not out.any(), refused
    assert host() == rcx.OK and total.value == int(stored_items.mix_items_numpy(x, good, pay, offs, 0)[1][-1])  # and the context still works


# ---- the host-buffer call and the way back -------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", sic.CODERS)
def test_host_call_equals_the_device_call(ctx, coder):
    items, payload, offsets = streams(ctx, coder, coder % 3)
    x, soffs = np.concatenate(items), sic.offsets_of(sic.LENGTHS)
    for gain in (0, 256):
        device = assert_mix(ctx, items, payload, offsets, gain, (coder, gain))
        mixed, moffs, flags = stored_items.mix_items(ctx, x, soffs, payload, offsets, gain)
        assert np.array_equal(mixed, device[0]) and np.array_equal(moffs, device[1]) and np.array_equal(flags, device[2])
    # items that begin past the front of the buffer
    shifted = np.concatenate([np.full(9, 0xEE, np.uint8), x])
    again = stored_items.mix_items(ctx, shifted, soffs + np.uint64(9), payload, offsets, 256)
    assert all(np.array_equal(a, b) for a, b in zip(again, (mixed, moffs, flags)))
    m, o, f = stored_items.mix_items(ctx, b"", [0], b"", [0])
    assert len(m) == 0 and o.tolist() == [0] and len(f) == 0
    m, o, f = stored_items.mix_items(ctx, b"", [0, 0, 0], b"", [0, 0, 0], 65535)
    assert len(m) == 0 and o.tolist() == [0, 0, 0] and f.tolist() == [0, 0]
    # a destination that is too small: the size comes back with the status
    size, small = rcx.C.c_uint64(), np.zeros(16, np.uint8)
    pay, offs = np.ascontiguousarray(payload), np.ascontiguousarray(offsets, dtype=np.uint64)
    st = stored_items.lib().rcx_stored_mix_items(ctx._h, x.ctypes.data, soffs.ctypes.data, len(items), pay.ctypes.data, len(pay), offs.ctypes.data, 0,
                                                 small.ctypes.data, 16, rcx.C.byref(size), None, None)
    assert st == rcx.E_CAPACITY and size.value == int(stored_items.mix_items_numpy(x, soffs, payload, offsets, 0)[1][-1]) and not small.any()


@pytest.mark.parametrize("coder", sic.CODERS)
def test_round_trip_through_the_stored_decode(ctx, coder):
    items, payload, offsets = streams(ctx, coder, 0)
    mixed, moffs, flags = assert_mix(ctx, items, payload, offsets, 0, coder, dst_offset=3)
    assert flags.any() and not flags[np.array(sic.LENGTHS) > 0].all(), "both kinds of stream"
    lengths = np.array(sic.LENGTHS, np.uint64)
    picks = {"all": None, "repeated": [13, 5, 13, 0, 0, 5, 5], "unordered": list(range(15, -1, -1)), "a subset": [12, 1, 8, 7], "only stored": list(np.flatnonzero(flags)[::-1]),
             "only empty": [0, 14], "empty": []}
    for k, (name, pick) in enumerate(picks.items()):
        comp = Guarded(len(mixed), sic.OFFSETS[k % 5], mixed, salt=4)
        offs = table(moffs, 5)
        doffs = rcx.item_offsets(lengths if pick is None else lengths[np.asarray(pick, dtype=np.int64)])
        out = Guarded(int(doffs[-1]), sic.OFFSETS[(k + 2) % 5], salt=6)
        stored.decode_device(ctx, comp.view, len(mixed), offs.view.view(torch.int64), flags, doffs, out.view, pick=pick, coder=coder)
        assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK, name
        comp.check(0, "decode comp")
        out.check(int(doffs[-1]), "decode dst")
        flat = out.view.cpu().numpy()
        for j, i in enumerate(range(len(items)) if pick is None else pick):
            assert np.array_equal(flat[int(doffs[j]): int(doffs[j + 1])], items[i]), (name, j, i)


# ---- containers --------------------------------------------------------------------------------------------------------------
def typed_batch():
    """Items of mixed widths and predictors: floats whose low planes no coder shrinks, sorted keys, small records, bytes, an
    empty item, and one of a single element."""
    rs = np.random.RandomState(9)
    floats = (rs.randn(3000) * 0.02).astype("<f4").view(np.uint8)
    half = (rs.randn(5000) * 0.02).astype("<f2").view(np.uint8)
    keys = np.sort(rs.randint(0, 1 << 40, 2000)).astype("<i8").view(np.uint8)
    return [(floats, 4, None), (keys, 8, "delta"), (rs.randint(0, 256, 16).astype(np.uint8), 1, None), (half[:-1], 2, None), (np.zeros(0, np.uint8), 4, "zigzag"),
            (sc.zipf_bytes(rs, 3000), 1, None), (keys[:8 * 300 + 3], 8, "zigzag"), (floats[:4], 4, "delta"), (rs.randint(0, 256, 2051).astype(np.uint8), 2, None)]


def pack_batch(ctx, coder, **kw):
    items = typed_batch()
    return container.pack_typed_items([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], coder, ctx, **kw)


@pytest.mark.parametrize("coder", sic.CODERS)
def test_pack_typed_items_and_unpack(ctx, coder):
    raw = [it[0].tobytes() for it in typed_batch()]
    for checksum in (False, True):
        today = container.parse_typed_items(pack_batch(ctx, coder, checksum=checksum, directory=b"carried"))
        blob = pack_batch(ctx, coder, checksum=checksum, directory=b"carried", stored=True)
        c = container.parse_typed_items(blob)
        assert blob[4] == 2 and c["flags"] == (6 if checksum else 4) and c["directory"] == b"carried"
        # the rule on what was coded, sub-item by sub-item; a kept stream is today's, a stored one is as long as its sub-item
        sizes, sub = np.diff(today["offsets"].astype(np.int64)), today["sub_lengths"].astype(np.int64)
        want = np.asarray(stored.is_stored(sizes, sub, 0)) & (sub > 0)
        assert np.array_equal(c["stored"], want) and want.any() and not want.all()
        assert np.array_equal(np.diff(c["offsets"].astype(np.int64)), np.where(want, sub, sizes))
        for k in np.flatnonzero(~want):
            assert np.array_equal(c["payload"][int(c["offsets"][k]): int(c["offsets"][k + 1])], today["payload"][int(today["offsets"][k]): int(today["offsets"][k + 1])])
        assert len(c["payload"]) <= sum(len(r) for r in raw) and len(c["payload"]) < len(today["payload"])
        if checksum:  # the CRC of the split text, as without the option
            assert np.array_equal(c["crcs"], today["crcs"])
        assert container.unpack_typed_items(blob, ctx=ctx) == raw and container.unpack_typed_items(blob, ctx=ctx, verify=False) == raw
        for pick in ([0], [3, 0], [8, 7, 6, 5, 4, 3, 2, 1, 0], [1, 1, 3, 1], [4], [2, 4, 2], []):
            assert container.unpack_typed_items(blob, pick, ctx) == [raw[k] for k in pick], (checksum, pick)
    # a fraction: more sub-items stored, never fewer
    more = container.parse_typed_items(pack_batch(ctx, coder, stored=0.3))["stored"]
    assert bool((more >= want).all()) and np.array_equal(more, np.asarray(stored.is_stored(sizes, sub, stored.gain_q16(0.3))) & (sub > 0))


@pytest.mark.parametrize("coder", sic.CODERS)
def test_width_1_is_the_stored_item_container(ctx, coder):
    items = sic.batch(sic.LENGTHS[:13] + (0, 7), 0)  # (without the 64 KiB item: quick)
    raw = [x.tobytes() for x in items]
    blob = container.pack_typed_items(items, widths=1, coder=coder, ctx=ctx, stored=True)
    plain = container.pack_items(items, coder, ctx)
    c, p = container.parse_typed_items(blob), container.parse_items(plain)
    assert container.unpack_typed_items(blob, ctx=ctx) == container.unpack_items(plain, ctx=ctx) == raw
    assert container.unpack_typed_items(blob, [12, 3, 3, 0], ctx) == container.unpack_items(plain, [12, 3, 3, 0], ctx)
    # its streams are the mix of the item container's
    want = stored_items.mix_items_numpy(np.concatenate(items), sic.offsets_of([len(x) for x in items]), p["payload"], p["offsets"], 0)
    assert np.array_equal(c["payload"], want[0]) and np.array_equal(c["offsets"], want[1]) and np.array_equal(c["stored"], want[2] != 0)


def test_nothing_stored_is_todays_container(ctx):
    items = [sc.shrinking_bytes(n, seed=n) for n in (4096, 5000, 8192)] + [np.zeros(0, np.uint8)]
    steps = (np.arange(5 * 4096, dtype=np.int32) // 1024)
    for coder in sic.CODERS:
        for checksum in (False, True):
            today = container.pack_typed_items(items, widths=1, coder=coder, ctx=ctx, checksum=checksum)
            assert container.pack_typed_items(items, widths=1, coder=coder, ctx=ctx, checksum=checksum, stored=True) == today and today[4] == 1
    for predict in (None, "delta"):
        today = container.pack_tensors({"steps": steps}, block=4096, predict=predict, ctx=ctx, checksum=True)
        assert container.pack_tensors({"steps": steps}, block=4096, predict=predict, ctx=ctx, checksum=True, stored=True) == today and today[4] == 1


@pytest.mark.parametrize("coder", sic.CODERS)
def test_uniform_items_never_grow(ctx, coder):
    rs = np.random.RandomState(coder)
    items = [rs.randint(0, 256, int(n)).astype(np.uint8) for n in rs.randint(16, 4097, 60)] + sic.zipf_batch(40, 16)
    total = sum(len(x) for x in items)
    blob = container.pack_typed_items(items, widths=1, coder=coder, ctx=ctx, stored=True)
    today = container.pack_typed_items(items, widths=1, coder=coder, ctx=ctx)
    c = container.parse_typed_items(blob)
    print(coder, total, len(container.parse_typed_items(today)["payload"]), len(c["payload"]))
    assert len(c["payload"]) <= total < len(container.parse_typed_items(today)["payload"]) and bool(c["stored"].all())
    assert container.unpack_typed_items(blob, ctx=ctx) == [x.tobytes() for x in items]


def test_a_flipped_byte_in_a_stored_sub_item(ctx):
    raw = [it[0].tobytes() for it in typed_batch()]
    blob = pack_batch(ctx, 0, checksum=True, stored=True)
    c = container.parse_typed_items(blob)
    k = int(c["sub_first"][0])  # the lowest mantissa plane of the floats
    assert c["stored"][k]
    bad = bytearray(blob)
    bad[len(blob) - len(c["payload"]) + int(c["offsets"][k]) + 100] ^= 0x10
    bad = bytes(bad)
    for call in (lambda: container.unpack_typed_items(bad, ctx=ctx), lambda: container.unpack_typed_items(bad, [5, 0, 1], ctx)):
        with pytest.raises(container.ChecksumError) as e:
            call()
        assert (e.value.kind, e.value.index) == ("item", 0)
    others = list(range(1, len(raw)))
    assert container.unpack_typed_items(bad, others, ctx) == [raw[j] for j in others]  # the items beside it still decode
    got = container.unpack_typed_items(bad, ctx=ctx, verify=False)
    assert got[0] != raw[0] and got[1:] == raw[1:] and sum(a != b for a, b in zip(got[0], raw[0])) == 1  # a copy: one byte of one element


@pytest.mark.parametrize("coder", (0, 3))
def test_pack_tensors_carries_the_streams_of_pack_typed(ctx, coder):
    block, gain = 4096, 256 / 65536
    torch.manual_seed(14)
    named = {"half": (torch.randn(2 * block, device="cuda") * 0.02).to(torch.bfloat16), "single": torch.randn(2 * block, device="cuda") * 0.02}
    for checksum in (False, True):
        blob = container.pack_tensors(named, block=block, coder=coder, ctx=ctx, checksum=checksum, stored=gain)
        c = container.parse_typed_items(blob)
        assert blob[4] == 2 and c["nitems"] == 4 and c["nsub"] == 2 * 2 + 2 * 4
        entries = {e["name"]: e for e in container.parse_tensor_directory(c["directory"], c["nitems"])}
        for name, t in named.items():
            typed = container.parse_typed(container.pack_typed(t, None, block, coder, ctx, checksum=checksum, stored=gain))
            first = int(c["sub_first"][entries[name]["first"]])
            assert typed["stored"] is not None and typed["stored"].any()
            for b in range(typed["nblocks"]):  # stream for stream
                got = c["payload"][int(c["offsets"][first + b]): int(c["offsets"][first + b + 1])]
                assert np.array_equal(got, typed["payload"][int(typed["offsets"][b]): int(typed["offsets"][b + 1])]), (name, b)
                assert c["stored"][first + b] == typed["stored"][b] and (not checksum or c["crcs"][first + b] == typed["crcs"][b])
            back = container.unpack_tensors(blob, names=[name], device="cuda", ctx=ctx)
            assert list(back) == [name] and back[name].is_cuda and torch.equal(back[name], t)
        back = container.unpack_tensors(blob, ctx=ctx)
        assert all(torch.equal(back[n], t.cpu()) for n, t in named.items())
