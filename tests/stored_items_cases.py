"""What the stored-item tests share (tests/test_stored_items_cpu.py, tests/test_gpu_stored_items.py): the batches, their bytes,
the CPU oracle's stream of every item, and the sub-items of the typed buffers cut as pack_tensors cuts them.  Not a test file."""
import numpy as np

import stats_cases
import stored_cases as sc
import typed_items_cases as tc
from cpprcoder_amd import typed_items

CODERS = sc.CODERS
GAINS = sc.GAINS
OFFSETS = sc.OFFSETS
COPY_SHORT = 1024  # RCX_COPY_SHORT: an item of at most this many bytes is a wave's entry, a longer one a workgroup's

# 1024 / 1025: the border between the two kinds of entry; 12 288 bytes = 3 * 256 pieces of 16 is where the workgroup's unrolled
# copy loop begins (12 287 below it, 12 305 one piece and a byte above, 16 389 = 4 * 256 pieces and 5); two empty items
LENGTHS = (0, 1, 15, 16, 17, 100, 1023, 1024, 1025, 4096, 12287, 12305, 16389, 65536, 0, 7)
TYPED = ("bf16", "fp32", "sorted_keys", "indices")  # the four buffers of the sizes that are pinned; sorted_keys with delta


def offsets_of(lengths, base=0):
    offs = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(np.asarray(lengths, dtype=np.uint64), out=offs[1:])
    return offs + np.uint64(base)


def item_bytes(length, kind, rs):
    """kind 0 uniform (no coder shrinks it), 1 Zipf (every coder does, once it is long enough), 2 one repeated byte."""
    if kind % 3 == 0:
        return rs.randint(0, 256, length).astype(np.uint8)
    if kind % 3 == 1:
        return sc.zipf_bytes(rs, length)
    return np.full(length, 0x41, np.uint8)


def batch(lengths=LENGTHS, first_kind=0, seed=3):
    """The items of `lengths`, their contents rotating through uniform, Zipf and one repeated byte from `first_kind` on, so that
    stored and kept entries of both kinds meet in one call."""
    rs = np.random.RandomState(seed)
    return [item_bytes(int(n), first_kind + i, rs) for i, n in enumerate(lengths)]


def ragged_items(seed=21, count=40):
    """Items of 0 .. 5000 bytes of all three kinds, three empty ones among them."""
    rs = np.random.RandomState(seed)
    lengths = [int(v) for v in rs.randint(1, 5000, count)]
    for at in (0, 7, count - 1):
        lengths[at] = 0
    lengths[3], lengths[4] = 16, 64
    return batch(lengths, 1, seed)


def zipf_batch(count=200, length=16, seed=5):
    """The issue's records: `count` items of `length` Zipf bytes."""
    rs = np.random.RandomState(seed)
    return [sc.zipf_bytes(rs, length) for _ in range(count)]


def oracle_item_streams(oracle, items, coder):
    """The CPU oracle's stream of every item on its own -> (payload, offsets); an item of length 0 has no stream."""
    streams = []
    for x in items:
        if len(x) == 0:
            streams.append(np.zeros(0, np.uint8))
            continue
        slots, sizes = oracle.encode_blocks(x, len(x), coder=coder)
        streams.append(slots[0, : int(sizes[0])].copy())
    return (np.concatenate(streams) if streams else np.zeros(0, np.uint8)), offsets_of([len(s) for s in streams])


def typed_sub_items(block):
    """The four typed buffers, each cut into superblock items as pack_tensors cuts it and split -> (the split text of all four
    back to back, the offsets of its sub-items).  A MiB is a whole number of superblocks at every width, so every sub-item is
    one whole block of the split text."""
    texts, lengths = [], []
    for name in TYPED:
        x, width = stats_cases.typed_bytes(name)
        lens, widths, preds = tc.superblock_items(len(x), width, block, tc.DELTA if name == "sorted_keys" else tc.NONE)
        offs = offsets_of(lens)
        texts.append(typed_items.split_numpy(x, offs, widths, preds))
        lengths += [int(v) for v in np.diff(typed_items.sub_offsets_numpy(offs, widths).astype(np.int64))]
    assert all(n == block for n in lengths)
    return np.concatenate(texts), offsets_of(lengths)
