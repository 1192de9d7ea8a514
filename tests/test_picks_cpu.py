"""The planner of rcx_decode_picks_device as cpprcoder_amd/picks.py restates it in numpy (include/rcx_picks.h): which entries
are valid, which are copied, what is latched and at which position -- on crafted tables with one entry of every kind; its
work order against the host planner's (rcx_items_plan); and what the binding and the library refuse without a device.
No GPU here: tests/test_gpu_picks.py holds the kernels to the same model."""
import numpy as np
import pytest

from cpprcoder_amd import picks, rcx

MAX_LEN = 5000
# six streams; 2 and 4 are stored (their streams are as long as their items), 5 is stored but its stream is one byte short
LENGTHS = np.array([100, 0, 700, 5000, 2000, 300], dtype=np.uint64)
STORED = np.array([0, 0, 1, 0, 1, 1], dtype=np.uint8)
SIZES = np.array([60, 0, 700, 3100, 2000, 299], dtype=np.uint64)
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
DST_CAP = 20000


def plan(pick, at, length, count, stored=STORED, max_len=MAX_LEN, nstreams=6, dst_cap=DST_CAP):
    return picks.plan_numpy(pick, at, length, count, max_len, nstreams, dst_cap, stored=stored, comp_offsets=OFFSETS if stored is not None else None,
                            comp_size=int(OFFSETS[-1]) if stored is not None else None)


def good_tables():
    """0: coded, 1: stored short, 2: coded long, 3: stored long, 4: a repeat of 0, 5: length 0 with a pick that names nothing"""
    pick = np.array([0, 2, 3, 4, 0, 77], dtype=np.uint64)
    length = np.array([100, 700, 5000, 2000, 100, 0], dtype=np.uint64)
    at = np.array([0, 100, 800, 5800, 7800, 1 << 62], dtype=np.uint64)
    return pick, at, length


def test_valid_tables_route_and_latch_nothing():
    pick, at, length = good_tables()
    p = plan(pick, at, length, 6)
    assert p["count"] == 6 and p["status"] == rcx.OK and p["position"] is None
    assert list(p["route"]) == [picks.CODED, picks.STORED_SHORT, picks.CODED, picks.STORED_LONG, picks.CODED, picks.NONE]
    assert p["bins"][0] == p["bins"][4] == picks.bin_of(100) and p["bins"][2] == picks.bin_of(5000)
    assert p["bins"][3] == picks.CODED_BINS and p["bins"][1] == picks.CODED_BINS + 1 and p["bins"][5] == -1
    # without flags every pick is coded
    q = plan(pick, at, length, 6, stored=None)
    assert list(q["route"]) == [picks.CODED] * 5 + [picks.NONE] and q["status"] == rcx.OK


@pytest.mark.parametrize("kind,entry,status", [
    ("bad pick", (6, 0, 10), rcx.E_CORRUPT),
    ("over-long", (3, 0, MAX_LEN + 1), rcx.E_CORRUPT),
    ("past dst_cap", (0, DST_CAP - 99, 100), rcx.E_CAPACITY),
    ("at past dst_cap, sum wraps", (0, (1 << 64) - 50, 100), rcx.E_CAPACITY),
    ("stored length mismatch", (5, 0, 300), rcx.E_CORRUPT),
    ("stored, wrong length asked", (2, 0, 699), rcx.E_CORRUPT),
])
@pytest.mark.parametrize("where", [1, 4])
def test_one_bad_entry_is_skipped_and_named(kind, entry, status, where):
    pick, at, length = good_tables()
    good = plan(pick, at, length, 6)
    pick[where], at[where], length[where] = entry
    p = plan(pick, at, length, 6)
    assert (p["status"], p["position"]) == (status, where), kind
    assert p["route"][where] == picks.NONE and p["bins"][where] == -1
    others = [k for k in range(6) if k != where]
    assert np.array_equal(p["route"][others], good["route"][others]) and np.array_equal(p["bins"][others], good["bins"][others])


def test_corrupt_outranks_capacity_and_the_lowest_position_is_named():
    pick, at, length = good_tables()
    at[1] = DST_CAP        # capacity at 1
    pick[3] = 6            # corrupt at 3
    p = plan(pick, at, length, 6)
    assert (p["status"], p["position"]) == (rcx.E_CORRUPT, 1)
    # an over-long entry that also leaves dst_cap is corrupt: the rules apply in the header's order
    pick, at, length = good_tables()
    length[2], at[2] = MAX_LEN + 1, DST_CAP
    assert plan(pick, at, length, 6)["status"] == rcx.E_CORRUPT


def test_a_length_of_zero_is_not_looked_at():
    pick = np.array([99, 0], dtype=np.uint64)
    p = plan(pick, np.array([1 << 63, 0], dtype=np.uint64), np.array([0, 100], dtype=np.uint64), 2)
    assert p["status"] == rcx.OK and list(p["route"]) == [picks.NONE, picks.CODED]


@pytest.mark.parametrize("count,meant,status,position", [(0, 0, rcx.OK, None), (3, 3, rcx.OK, None), (6, 6, rcx.OK, None),
                                                          (7, 6, rcx.E_CAPACITY, 6), (1 << 63, 6, rcx.E_CAPACITY, 6)])
def test_the_count(count, meant, status, position):
    pick, at, length = good_tables()
    p = plan(pick, at, length, count)
    assert (p["count"], p["status"], p["position"]) == (meant, status, position)
    assert not p["route"][meant:].any() and p["route"][:min(meant, 5)].all()


def test_entries_past_the_count_are_not_read():
    pick, at, length = good_tables()
    full = plan(pick, at, length, 2)
    pick[2:], at[2:], length[2:] = 1 << 63, 1 << 63, 1 << 63
    p = plan(pick, at, length, 2)
    assert p["status"] == rcx.OK and np.array_equal(p["route"], full["route"]) and np.array_equal(p["bins"], full["bins"])
    # a bad entry in front of a count above max_pick: the lowest position wins, corrupt outranks capacity
    pick, at, length = good_tables()
    pick[0] = 6
    assert (plan(pick, at, length, 9)["status"], plan(pick, at, length, 9)["position"]) == (rcx.E_CORRUPT, 0)


def test_bins_are_the_work_order():
    """Ascending bins are descending lengths; below 512 a bin is one length, above it spans less than 1/256 of its lengths."""
    lengths = list(range(1, 1200)) + [4095, 4096, 4097, 65535, 65536, 65537, (1 << 24) - 256]
    bins = [picks.bin_of(n) for n in lengths]
    assert all(0 <= b < picks.CODED_BINS for b in bins)
    assert all(b1 >= b2 for b1, b2 in zip(bins, bins[1:]))
    assert len({picks.bin_of(n) for n in range(1, 512)}) == 511
    for n in (512, 1000, 4096, 70000, 1 << 20, (1 << 24) - 256):
        same = [m for m in range(n, min(n + n // 128 + 2, 1 << 24)) if picks.bin_of(m) == picks.bin_of(n)]
        assert 1 <= len(same) <= n // 256 + 1, n
    for bad in (0, 1 << 24):
        with pytest.raises(ValueError):
            picks.bin_of(bad)


@pytest.mark.parametrize("coder", (rcx.CODER_ADAPTIVE, rcx.CODER_RANS8))
def test_valid_contiguous_tables_agree_with_the_host_planner(coder):
    """All items picked in order to back-to-back outputs: the entries with a route are rcx_items_plan's work entries, with its
    lengths, and the host's order (longest first) never goes down in bins."""
    rs = np.random.RandomState(5)
    lengths = np.concatenate([[0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 70000, 0], rs.randint(0, 5001, 300)]).astype(np.uint64)
    offs = rcx.item_offsets(lengths)
    order, _, _ = rcx.items_plan(offs, coder)
    n = len(lengths)
    p = picks.plan_numpy(np.arange(n), offs[:-1], lengths, n, 70000, n, int(offs[-1]))
    assert p["status"] == rcx.OK
    routed = np.flatnonzero(p["route"])
    assert np.array_equal(np.sort(order.astype(np.int64)), routed) and np.all(p["route"][routed] == picks.CODED)
    assert np.array_equal(lengths[order], np.sort(lengths[routed])[::-1])
    assert np.all(np.diff(p["bins"][order]) >= 0)


def test_plan_numpy_refuses_tables_that_do_not_match():
    with pytest.raises(ValueError):
        picks.plan_numpy([0, 1], [0], [1, 1], 2, 10, 2, 100)
    with pytest.raises(ValueError):
        picks.plan_numpy([0], [0], [1], 1, 10, 2, 100, stored=[1, 0])  # flags without the streams' table


# ---- what needs no device ----------------------------------------------------------------------------------------------------
def test_scratch_formula():
    """24 bytes an entry, the planner's two counter tables and four words, and max_pick + 1 redo marks (include/rcx_picks.h)."""
    for coder in (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC, rcx.CODER_RANS, rcx.CODER_RANS8):
        for max_pick in (1, 1000, 200_000, picks.MAX_PICK):
            assert picks.scratch_bytes(max_pick, 4096, coder) == max_pick * 24 + (2 * picks.BINS + 4) * 4 + (max_pick + 1) * 4
    assert picks.BINS == 4354
    assert picks.scratch_bytes(0, 4096) == 0
    assert picks.scratch_bytes(picks.MAX_PICK + 1, 4096) == 0
    assert picks.scratch_bytes(10, rcx.MAX_BLOCK + 1) == 0
    assert picks.scratch_bytes(10, 4096, coder=9) == 0


def test_the_library_exports_the_header():
    lib = picks.lib()
    for name in picks.EXPORTS:
        getattr(lib, name)


def test_argument_errors_without_a_device():
    """RCX_E_ARG before anything is touched: no context; and the binding refuses tables that are not on the device, not 64-bit
    integers, or too short, before it calls anything."""
    lib = picks.lib()
    assert lib.rcx_picks_reserve(None, 0, 10, 100) == rcx.E_ARG
    assert lib.rcx_decode_picks_device(None, 0, None, 0, None, 0, None, None, None, None, None, 1, 16, None, 0, None) == rcx.E_ARG
    assert lib.rcx_decode_picks(None, 0, None, 0, None, 0, None, None, None, None, 0, 16, None, 0) == rcx.E_ARG
    torch = pytest.importorskip("torch")

    class NoContext:
        _h = None

    t8 = torch.zeros(4, dtype=torch.int64)
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        picks.decode_device(NoContext(), u8, 64, t8, t8, t8, t8, t8, u8, 100)
    with pytest.raises(ValueError, match="max_pick"):
        picks.decode_device(NoContext(), u8, 64, t8, t8, t8, t8, t8, u8, 100, max_pick=1 << 31)
    with pytest.raises(ValueError):
        picks.decode(NoContext(), u8.numpy(), [0, 64], [0], [0, 1], [5], 16, np.zeros(16, np.uint8))
    with pytest.raises(ValueError):
        picks.decode(NoContext(), u8.numpy(), [0, 64], [0], [0], [5], 16, np.zeros(16, np.int32))
