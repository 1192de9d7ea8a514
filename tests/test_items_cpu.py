"""The item calls (include/rcx.h, "Item calls") as far as they go without a GPU: the exports, the pure bound, the
host-side planner (work order, length classes, scratch) and the item container's header."""
import numpy as np
import pytest

from cpprcoder_amd import container

NEW_SYMBOLS = ("rcx_encode_items_bound", "rcx_items_plan", "rcx_ctx_scratch_bytes", "rcx_encode_items_device", "rcx_decode_items_device",
               "rcx_encode_items", "rcx_decode_items")


@pytest.fixture(scope="module")
def rcx():
    from cpprcoder_amd import build, rcx as r
    build.build()
    r.lib()
    return r


def test_library_exports_the_item_calls(rcx):
    for name in NEW_SYMBOLS:
        assert name in rcx.EXPORTS and getattr(rcx.lib(), name) is not None
    assert rcx.lib().rcx_version() == 300


def test_items_bound_is_the_sum_of_the_block_bounds(rcx):
    rs = np.random.RandomState(5)
    lengths = np.concatenate([[0, 1, 2, 15, 16, 17, 0, 65536, 65537, 200_000, 0, rcx.MAX_BLOCK], rs.randint(0, 50_000, 300)])
    offs = rcx.item_offsets(lengths)
    for coder in range(4):
        want = sum(rcx.block_bound(int(n), coder) for n in lengths if n)
        assert rcx.encode_items_bound(offs, coder) == want
    assert rcx.encode_items_bound(rcx.item_offsets([0, 0, 0])) == 0
    assert rcx.encode_items_bound(np.zeros(1, np.uint64)) == 0
    # a bad table has no bound, and no plan
    assert rcx.encode_items_bound(np.array([0, 10, 5], np.uint64)) == 0
    assert rcx.encode_items_bound(np.array([0, rcx.MAX_BLOCK + 1], np.uint64)) == 0
    for bad in (np.array([0, 10, 5], np.uint64), np.array([0, rcx.MAX_BLOCK + 1], np.uint64)):
        with pytest.raises(rcx.RcxError) as e:
            rcx.items_plan(bad)
        assert e.value.status == rcx.E_ARG


def test_planner_on_a_skewed_batch(rcx):
    """One item of 4 MiB among 200 000 of 64 bytes: a single stride of bound(longest) would ask for about 970 GB.  The
    planned scratch stays within 2 x the bound of the data + RCX_ITEM_SCRATCH_BYTES per item, and the work order is a
    bijection that starts with the long item."""
    lengths = np.full(200_001, 64, dtype=np.uint64)
    lengths[123_456] = 4 << 20
    offs = rcx.item_offsets(lengths)
    for coder in range(4):
        order, scratch, nclasses = rcx.items_plan(offs, coder)
        assert len(order) == len(lengths) and np.array_equal(np.sort(order), np.arange(len(lengths), dtype=np.uint32))
        assert order[0] == 123_456
        assert nclasses == 2
        bound = rcx.encode_items_bound(offs, coder)
        assert 0 < scratch <= 2 * bound + rcx.ITEM_SCRATCH_BYTES * len(lengths), (coder, scratch, bound)
        assert scratch < 2 * len(lengths) * rcx.block_bound(4 << 20, coder) // 100  # nowhere near one stride for all


def test_planner_orders_by_length_and_leaves_out_empty_items(rcx):
    rs = np.random.RandomState(11)
    lengths = np.exp(rs.uniform(0, np.log(300_000), 5000)).astype(np.uint64)
    lengths[rs.randint(0, 5000, 200)] = 0
    offs = rcx.item_offsets(lengths)
    order, scratch, nclasses = rcx.items_plan(offs)
    live = np.flatnonzero(lengths)
    assert np.array_equal(np.sort(order), live.astype(np.uint32))          # a bijection onto the items that have a stream
    assert np.all(np.diff(lengths[order].astype(np.int64)) <= 0)           # longest first
    same = np.flatnonzero(np.diff(lengths[order].astype(np.int64)) == 0)
    assert np.all(order[same] < order[same + 1])                           # the caller's order among equals
    assert 1 <= nclasses <= 21                                              # 16, 32, ... 2^24
    assert scratch <= 2 * rcx.encode_items_bound(offs) + rcx.ITEM_SCRATCH_BYTES * len(lengths)
    assert rcx.items_plan(rcx.item_offsets([0, 0]))[1] == 0 and len(rcx.items_plan(np.zeros(1, np.uint64))[0]) == 0


def test_item_container_header_round_trip_and_rejections():
    lengths = np.array([100, 0, 7, 70_000], np.uint64)
    offs = np.array([0, 60, 60, 75, 40_000], np.uint64)
    blob = container.item_header_bytes(2, lengths, offs) + bytes(40_000)
    c = container.parse_items(blob)
    assert (c["coder"], c["nitems"]) == (2, 4) and len(c["payload"]) == 40_000
    assert np.array_equal(c["lengths"], lengths) and np.array_equal(c["offsets"], offs)
    empty = container.parse_items(container.item_header_bytes(0, [], [0]))
    assert empty["nitems"] == 0 and len(empty["payload"]) == 0
    for damaged in (b"RCXB" + blob[4:], blob[:-1], blob + b"x", blob[:40], blob[:10]):
        with pytest.raises(container.ContainerError):
            container.parse_items(damaged)
    for at, value in ((4, 2), (5, 9), (6, 1), (7, 1)):  # version, coder, either byte of the flags
        bad = bytearray(blob)
        bad[at] = value
        with pytest.raises(container.ContainerError):
            container.parse_items(bytes(bad))
    with pytest.raises(container.ContainerError):  # an empty item with a stream
        container.parse_items(container.item_header_bytes(0, [5, 0], [0, 20, 30]) + bytes(30))
    with pytest.raises(container.ContainerError):  # an item with no stream
        container.parse_items(container.item_header_bytes(0, [5, 5], [0, 20, 20]) + bytes(20))
    with pytest.raises(container.ContainerError):  # a decreasing table
        container.parse_items(container.item_header_bytes(0, [5, 5], [0, 20, 10]) + bytes(10))
    with pytest.raises(container.ContainerError):
        container.item_header_bytes(0, [5, 5], [0, 20])
    with pytest.raises(container.ContainerError):
        container.item_header_bytes(0, [(1 << 24) - 255], [0, 20])
    # the two containers do not read each other's files
    with pytest.raises(container.ContainerError):
        container.parse(blob)
    with pytest.raises(container.ContainerError):
        container.parse_items(container.header_bytes(0, 4096, 100, np.array([0, 5], np.uint64)) + bytes(5))


def test_block_container_still_rejects_unknown_flags():
    bad = bytearray(container.header_bytes(0, 4096, 100, np.array([0, 5], np.uint64)) + bytes(5))
    bad[6] = 2  # flag bit 1
    with pytest.raises(container.ContainerError):
        container.parse(bytes(bad))
    bad[6] = 3
    with pytest.raises(container.ContainerError):
        container.parse(bytes(bad))
