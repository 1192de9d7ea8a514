"""What tests/test_encode_picks_cpu.py and tests/test_gpu_encode_picks.py share: the length sets and crafted tables of
rcx_encode_picks_device (include/rcx_encode_picks.h), and the checks of a layout that cpprcoder_amd/encode_picks.py's plan_numpy
states.  No torch, no GPU, nothing of the reference's tree."""
import numpy as np

from cpprcoder_amd import encode_picks as ep, rcx

PAST = 1 << 63  # what table entries at or behind the count are filled with
TOP = 17        # class edges up to 2^TOP: no item above 2^17 + 1 bytes


def edge_lengths():
    """Both sides of every class edge up to 2^17 -- 16, 17, 32, 33, ... 2^17, 2^17 + 1 -- and 1, 15 and 0."""
    return [0, 1, 15] + [n for e in range(4, TOP + 1) for n in (1 << e, (1 << e) + 1)]


def skew_lengths(seed=5):
    """One item of 2^17 + 1 bytes among 300 of 1 .. 64: what must not cost max_items x bound(max_len)."""
    rs = np.random.RandomState(seed)
    lengths = list(rs.randint(1, 65, 300))
    lengths.insert(137, (1 << TOP) + 1)
    return lengths


def padding_lengths(n):
    """A class of exactly n entries (65 .. 128 bytes) between two others: the unit padding at 63, 64 and 65."""
    rs = np.random.RandomState(n)
    return list(rs.randint(65, 129, n)) + [40, 33, 700, 513, 600]


def back_to_back(lengths, gap=0, first=0):
    """-> (src_at uint64[], the size of the source): item k begins `gap` bytes behind item k - 1."""
    at, cursor = np.zeros(len(lengths), np.uint64), first
    for k, n in enumerate(lengths):
        at[k] = cursor
        cursor += int(n) + gap
    return at, cursor


def every_residue(lengths):
    """-> (src_at, size): each item starts at the next residue mod 16 of the one before (items overlap nothing)."""
    at, cursor = np.zeros(len(lengths), np.uint64), 0
    for k, n in enumerate(lengths):
        cursor += (k % 16 - cursor) % 16
        at[k] = cursor
        cursor += int(n)
    return at, cursor


BAD = {  # kind -> (src_at, src_len) of the bad entry, given src_cap and max_len
    "length above max_len": lambda cap, max_len: (0, max_len + 1),
    "position past src_cap": lambda cap, max_len: (cap + 1, 1),
    "end past src_cap": lambda cap, max_len: (cap - 10, 11),
    "a sum that would wrap": lambda cap, max_len: ((1 << 64) - 5, 10),
}
BAD_STATUS = {"length above max_len": rcx.E_CORRUPT, "position past src_cap": rcx.E_CAPACITY, "end past src_cap": rcx.E_CAPACITY,
              "a sum that would wrap": rcx.E_CAPACITY}


def check_layout(plan, lengths, coder):
    """The invariants of a layout: classes in order and each on a unit of its own, holes only at a class's end, strides the
    class's bound, slot bases disjoint and ascending, every live entry's slot inside slots_bytes."""
    units = plan["units"]
    assert plan["positions"] == 64 * len(units)
    assert [u[0] for u in units] == sorted(u[0] for u in units), "classes out of order"
    end = 0
    for i, (c, stride, base, live) in enumerate(units):
        assert stride == rcx.block_bound(ep.class_upper(c), coder)
        assert 1 <= live <= 64
        last_of_class = i + 1 == len(units) or units[i + 1][0] != c
        assert live == 64 or last_of_class, "a hole in front of a live entry of its class"
        assert plan["class_first"][c] <= 64 * i < plan["class_first"][c] + -(-plan["class_count"][c] // 64) * 64
        assert base == end, "slots overlap or leave a gap"
        end = base + live * stride
    assert end == plan["slots_bytes"]
    valid = plan["valid"]
    assert sum(u[3] for u in units) == int(valid.sum())
    for k in np.nonzero(valid)[0]:
        c = int(plan["klass"][k])
        assert ep.class_upper(c) >= int(lengths[k]) and (c == ep.CLASSES - 1 or ep.class_upper(c + 1) < int(lengths[k]))
