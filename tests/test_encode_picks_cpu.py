"""The planner of rcx_encode_picks_device as cpprcoder_amd/encode_picks.py restates it in numpy (include/rcx_encode_picks.h):
which entries are valid, their classes, the layout of the work order in units of 64 with the stride and slot base of each, what
is latched and where; the same against the host plan (rcx_items_plan); the scratch formula; the container that
pack_items_device's result writes; and what the library and the binding refuse without a device.  No GPU here:
tests/test_gpu_encode_picks.py holds the kernels to the same model."""
import numpy as np
import pytest

from cpprcoder_amd import container, encode_picks as ep, layout, rcx
from encode_picks_cases import BAD, BAD_STATUS, PAST, back_to_back, check_layout, edge_lengths, padding_lengths, skew_lengths

CODERS = (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC, rcx.CODER_RANS, rcx.CODER_RANS8)


def plan(at, length, count, max_len=5000, src_cap=1 << 20, max_bytes=1 << 30, coder=0):
    return ep.plan_numpy(at, length, count, max_len, src_cap, max_bytes, coder)


def test_one_entry_of_every_kind():
    """An over-long entry, one past src_cap, one whose end is, one whose sum would wrap, a length of 0 (whose position is not
    looked at), and two entries that name the same bytes."""
    cap = 10_000
    at = [0, 0, cap + 1, cap - 10, (1 << 64) - 5, PAST, 100, 100, cap - 7]
    ln = [100, 5001, 1, 11, 10, 0, 300, 300, 7]
    p = plan(at, ln, len(at), src_cap=cap)
    assert list(p["valid"]) == [True, False, False, False, False, False, True, True, True]
    assert p["status"] == rcx.E_CORRUPT and p["position"] == 1  # CORRUPT before CAPACITY, the lowest position of either
    assert p["total"] == 100 + 300 + 300 + 7 and not p["over"]
    assert p["klass"][6] == p["klass"][7] == ep.class_of(300) == 24 - 9 and p["klass"][8] == ep.CLASSES - 1 and p["klass"][1] == -1
    q = plan(at[2:], ln[2:], len(at) - 2, src_cap=cap)
    assert q["status"] == rcx.E_CAPACITY and q["position"] == 0
    for kind, make in BAD.items():
        a, n = make(cap, 5000)
        r = plan([0, a, 50], [10, n, 20], 3, src_cap=cap)
        assert (r["status"], r["position"]) == (BAD_STATUS[kind], 1) and list(r["valid"]) == [True, False, True], kind


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 1 << 40])
def test_the_count(count):
    """Entries at or behind the count are not read, whatever they hold; a count above max_items is max_items and CAPACITY there."""
    at, ln = [0, 10, 20, 30], [10, 10, 10, 10]
    meant = min(count, 4)
    at[meant:], ln[meant:] = [PAST] * (4 - meant), [PAST] * (4 - meant)
    p = plan(at, ln, count)
    assert p["count"] == meant and int(p["valid"].sum()) == meant and p["total"] == 10 * meant
    assert (p["status"], p["position"]) == ((rcx.E_CAPACITY, 4) if count > 4 else (rcx.OK, None))
    assert p["positions"] == (64 if meant else 0)


def test_max_bytes_exceeded():
    """The valid lengths sum to more than was promised: nothing is laid out, CAPACITY at the count; a skipped entry does not count."""
    at, ln = [0, 100, 200, 0], [100, 100, 100, 9999]
    assert not plan(at, ln, 4, max_bytes=300)["over"] and plan(at, ln, 4, max_bytes=300)["status"] == rcx.E_CORRUPT
    p = plan(at, ln, 3, max_bytes=299)
    assert p["over"] and p["positions"] == 0 and p["units"] == [] and (p["status"], p["position"]) == (rcx.E_CAPACITY, 3)
    p = plan(at, ln, 9, max_bytes=299)  # an over-long entry, a count above max_items and the total: CORRUPT first, the lowest position
    assert p["over"] and (p["status"], p["position"]) == (rcx.E_CORRUPT, 3)


def test_classes_and_bins_at_the_edges():
    """A class is (U / 2, U]; no bin spans two classes, bins ascend as lengths descend, and lengths below 513 have bins of their own."""
    for e in range(4, 24):
        assert ep.class_of(1 << e) == 24 - e and ep.class_of((1 << e) + 1) == 24 - e - 1
        assert ep.bin_of(1 << e) != ep.bin_of((1 << e) + 1)
        assert ep.class_upper(24 - e) == 1 << e
    assert ep.class_of(1) == ep.class_of(16) == 20 and ep.class_of(rcx.MAX_BLOCK) == 0 and ep.class_upper(0) == rcx.MAX_BLOCK
    assert ep.bin_of(rcx.MAX_BLOCK) == 0 and ep.bin_of(1) == ep.CODED_BINS - 1
    lengths = sorted(set(list(range(1, 1200)) + [n + d for e in range(10, 24) for n in (1 << e,) for d in (-1, 0, 1, 2)] + [rcx.MAX_BLOCK]))
    bins = [ep.bin_of(n) for n in lengths]
    assert all(a >= b for a, b in zip(bins, bins[1:])), "a longer entry in a later bin"
    assert len({ep.bin_of(n) for n in range(1, 514)}) == 513
    by_bin = {}
    for n in lengths:
        by_bin.setdefault(ep.bin_of(n), set()).add(ep.class_of(n))
    assert all(len(c) == 1 for c in by_bin.values()), "a bin that spans two classes"
    for bad in (0, rcx.MAX_BLOCK + 1):
        with pytest.raises(ValueError):
            ep.bin_of(bad)


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("name", ["edges", "skew", "pad63", "pad64", "pad65"])
def test_against_the_host_plan(coder, name):
    """The same lengths through rcx_items_plan: as many classes, the same classes along the host's work order (longest first),
    and the same slot memory -- so the same strides."""
    lengths = {"edges": edge_lengths() * 2, "skew": skew_lengths(), "pad63": padding_lengths(63), "pad64": padding_lengths(64),
               "pad65": padding_lengths(65)}[name]
    at, size = back_to_back(lengths)
    p = plan(at, lengths, len(lengths), max_len=(1 << 17) + 1, src_cap=size, coder=coder)
    assert p["status"] == rcx.OK
    order, scratch, nclasses = rcx.items_plan(rcx.item_offsets(lengths), coder)
    assert nclasses == int(np.count_nonzero(p["class_count"])) == len({u[0] for u in p["units"]})
    assert sorted(int(k) for k in order) == [int(k) for k in np.nonzero(p["valid"])[0]]
    assert [int(p["klass"][k]) for k in order] == sorted(int(c) for c in p["klass"][p["valid"]])
    nwork, n = len(order), len(lengths)
    host_slots = scratch - (nwork * 20 + n * 4 + 16) - 2 * 4 * (nwork + 1) - 256
    if coder in (rcx.CODER_RANS, rcx.CODER_RANS8):
        host_slots -= 4 * (nwork + 1)
    if coder == rcx.CODER_RANS:
        host_slots -= ep.RANS_MODEL_BYTES * nwork
    assert host_slots == p["slots_bytes"]
    check_layout(p, lengths, coder)


@pytest.mark.parametrize("coder", CODERS)
def test_the_planned_scratch_never_exceeds_the_formula(coder):
    """Seeded random length sets with sum(len) <= max_bytes: the layout's slots fit the formula's slot term, its positions the
    max_items + PAD the per-entry arrays are sized for; the layout invariants hold."""
    rs = np.random.RandomState(23 + coder)
    for trial in range(40):
        n = int(rs.randint(1, 400))
        top = int(rs.choice([1, 8, 16, 17, 100, 4096, 70_000, 1 << 20, rcx.MAX_BLOCK]))
        lengths = rs.randint(0, top + 1, n)
        if trial % 5 == 0:
            lengths[:] = top  # all at a class's upper end, or just past one
        at, size = back_to_back(lengths)
        p = plan(at, lengths, n, max_len=rcx.MAX_BLOCK, src_cap=size, max_bytes=int(lengths.sum()), coder=coder)
        assert p["status"] == rcx.OK and not p["over"]
        check_layout(p, lengths, coder)
        assert p["slots_bytes"] <= ep.slots_bound(n, int(lengths.sum()), coder), (trial, top)
        assert p["positions"] + 64 <= n + ep.PAD
        # (what the library reserves for the layout's positions and slots is the formula's)
        assert ep.scratch_formula(n, int(lengths.sum()), coder) == ep.scratch_bytes(n, top, int(lengths.sum()), coder)


def test_scratch_formula():
    """The library's answer is the header's closed formula: linear in max_items and in max_bytes, the same at two values of
    max_len, and far from max_items x bound(max_len) for one long item among many short ones."""
    for coder in CODERS:
        for max_items, max_bytes in ((1, 1), (1000, 1 << 20), (200_000, 1 << 30), (ep.MAX_ITEMS, 1 << 40)):
            got = ep.scratch_bytes(max_items, 4096, max_bytes, coder)
            assert got == ep.scratch_formula(max_items, max_bytes, coder) == ep.scratch_bytes(max_items, rcx.MAX_BLOCK, max_bytes, coder)
        f = lambda m, b: ep.scratch_bytes(m, 4096, b, coder)  # noqa: E731
        assert f(3000, 10_000) - f(2000, 10_000) == f(2000, 10_000) - f(1000, 10_000)
        assert f(1000, 30_000) - f(1000, 20_000) == f(1000, 20_000) - f(1000, 10_000)
        skew = f(200_001, (4 << 20) + 200_000 * 64)
        assert skew < 200_001 * rcx.block_bound(4 << 20, coder) // 100
    assert ep.scratch_bytes(0, 4096, 100) == 0
    assert ep.scratch_bytes(ep.MAX_ITEMS + 1, 4096, 100) == 0
    assert ep.scratch_bytes(10, rcx.MAX_BLOCK + 1, 100) == 0
    assert ep.scratch_bytes(10, 4096, 100, coder=9) == 0


def test_the_library_exports_the_header():
    lib = ep.lib()
    for name in ep.EXPORTS:
        getattr(lib, name)
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcx_encode_picks.h")).read()
    names = re.findall(r"^(?:int|uint64_t)\s+(rcx_\w+)\(", header, re.M)
    assert len(names) == 4 and set(names) == set(ep.EXPORTS), names
    from cpprcoder_amd import base_picks, picks, typed_picks
    assert len(rcx.EXPORTS) == 57 and not set(ep.EXPORTS) & (set(rcx.EXPORTS) | set(picks.EXPORTS) | set(typed_picks.EXPORTS) | set(base_picks.EXPORTS))


def test_argument_errors_without_a_device():
    """RCX_E_ARG before anything is touched: no context, a null table, max_len above RCX_MAX_BLOCK, max_items of 2^31, a coder
    that is none; and the binding refuses tables that are not on the device, not 64-bit integers, or too short, before it calls."""
    lib = ep.lib()
    assert lib.rcx_encode_picks_reserve(None, 0, 10, 100, 1000) == rcx.E_ARG
    assert lib.rcx_encode_picks_device(None, 0, None, 0, None, None, None, 1, 16, 16, None, 0, None, None) == rcx.E_ARG
    assert lib.rcx_encode_picks(None, 0, None, 0, None, None, 0, 16, None, 0, None, None) == rcx.E_ARG
    a = np.zeros(64, np.uint64)
    p = a.ctypes.data  # (a pointer that is not null; with a refusal nothing is read through it)
    for coder, max_items, max_len in ((9, 4, 16), (0, 1 << 31, 16), (0, 4, rcx.MAX_BLOCK + 1)):
        assert lib.rcx_encode_picks_reserve(p, coder, max_items, max_len, 1000) == rcx.E_ARG
        assert lib.rcx_encode_picks_device(p, coder, p, 64, p, p, p, max_items, max_len, 64, p, 64, p, None) == rcx.E_ARG
        assert lib.rcx_encode_picks(p, coder, p, 64, p, p, max_items, max_len, p, 64, p, p) == rcx.E_ARG
    for null in range(6):  # each pointer of the device call in turn
        ptrs = [p] * 6
        ptrs[null] = None
        src, at, ln, count, dst, offs = ptrs
        assert lib.rcx_encode_picks_device(p, 0, src, 64, at, ln, count, 4, 16, 64, dst, 64, offs, None) == rcx.E_ARG, null
    torch = pytest.importorskip("torch")

    class NoContext:
        _h = None

    t8 = torch.zeros(4, dtype=torch.int64)
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        ep.encode_device(NoContext(), u8, t8, t8, t8, u8, t8, 16, 64)
    with pytest.raises(ValueError, match="max_items"):
        ep.encode_device(NoContext(), u8, t8, t8, t8, u8, t8, 16, 64, max_items=1 << 31)
    with pytest.raises(ValueError, match="cuda"):
        container.pack_items_device(NoContext(), u8, t8, t8, t8, 4, 16, 64)
    with pytest.raises(ValueError):
        ep.encode(NoContext(), u8.numpy(), [0, 1], [5], 16)


@pytest.mark.parametrize("count", [0, 3, 5, 9])
def test_to_bytes_is_the_item_container(count):
    """PackedItems.to_bytes() over synthetic streams: max_items = 5 streams of which the first `count` are meant (the others
    empty, their lengths garbage) -> byte for byte layout.py's RCXI for the meant items, which parse_items reads back."""
    torch = pytest.importorskip("torch")

    class Synced:
        def sync_status(self):
            return (rcx.OK, 0xFFFFFFFF)

    meant = min(count, 5)
    lengths = np.array([100, 0, 7, 3000, 16], np.int64)
    sizes = np.array([40, 0, 11, 900, 20], np.int64)
    sizes[meant:] = 0
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    payload = (np.arange(2000) * 7 % 251).astype(np.uint8)
    d_len = torch.from_numpy(np.where(np.arange(5) < meant, lengths, -(1 << 63)))
    box = container.PackedItems(Synced(), 1, d_len, torch.tensor([count], dtype=torch.int64), 5, 3000, torch.from_numpy(payload), torch.from_numpy(offsets))
    blob = box.to_bytes()
    want = layout.item_header_bytes(1, lengths[:meant], offsets[: meant + 1]) + payload[: int(offsets[meant])].tobytes()
    assert blob == want
    c = layout.parse_items(blob)
    assert c["coder"] == 1 and c["nitems"] == meant and list(c["lengths"]) == list(lengths[:meant]) and c["crcs"] is None
    assert bytes(c["payload"]) == payload[: int(offsets[meant])].tobytes()
