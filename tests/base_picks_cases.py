"""What the device-planned base join's tests share (tests/test_base_picks_cpu.py, tests/test_gpu_base_picks.py): where the
entries of a batch of base_items_cases lie when the split text is packed, the destinations are scattered and the entries are
shuffled.  Not a test file."""
import numpy as np

import base_items_cases as bc


def scattered(lengths, rs):
    """Where each entry's bytes go: the entries take their places in a shuffled order, each start at the next residue mod 16
    with a gap of guard bytes in front of it -> (at uint64[], the size of the buffer)."""
    at = np.zeros(len(lengths), np.uint64)
    cursor = 0
    for r, k in enumerate(rs.permutation(len(lengths))):
        cursor += (r % 16 - cursor) % 16 + 16
        at[k] = cursor
        cursor += int(lengths[k])
    return at, cursor + 16


def parity_tables(case):
    """The tables of the parity test for a batch -> dict(offs: the packed split text's offsets; boffs, nbase: base_layout's;
    at, size: the scattered destinations; order: the shuffle of the entries)."""
    n = len(case["lengths"])
    rs = np.random.RandomState(n + 7)
    order = rs.permutation(n)
    boffs, nbase = bc.base_layout(case)
    at, size = scattered(case["lengths"], rs)
    return {"offs": bc.offsets_of(case), "boffs": boffs, "nbase": nbase, "at": at, "size": size, "order": order}
