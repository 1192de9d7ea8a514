"""What the stored-block tests share (tests/test_stored_cpu.py, tests/test_gpu_stored.py): the fixtures, the case lists and
the container builders.  Not a test file."""
import numpy as np

import planes_cases as pc

CODERS = (0, 1, 2, 3)
BLOCKS = (16, 100, 1024, 1040, 4096, 65536)  # 1024 / 1040: the copy kernel's border between a wave's entry and a workgroup's
OFFSETS = (0, 1, 3, 8, 15)
GAINS = (0, 256, 65535)
NBLOCKS = 6


def zipf_bytes(rs, n):
    """n bytes, value k with probability ~ 1 / (k + 1)."""
    p = 1.0 / np.arange(1, 257)
    return rs.choice(256, size=n, p=p / p.sum()).astype(np.uint8)


def mixed_bytes(block, tail=None, seed=7):
    """Six blocks: uniform, Zipf, uniform, one repeated byte, uniform, Zipf; the last one `tail` bytes long (block - 7 if None):
    blocks that no coder shrinks beside blocks that every coder does."""
    rs = np.random.RandomState(seed)
    parts = []
    for b in range(NBLOCKS):
        if b % 2 == 0:
            parts.append(rs.randint(0, 256, block).astype(np.uint8))
        elif b == 3:
            parts.append(np.full(block, 0x41, np.uint8))
        else:
            parts.append(zipf_bytes(rs, block))
    x = np.concatenate(parts)
    return x[: (NBLOCKS - 1) * block + (block - 7 if tail is None else tail)]


def shrinking_bytes(n, seed=11):
    """Two byte values, one nine times as frequent as the other: every coder shrinks every block of 2048 bytes or more
    (rANS takes 1032 bytes for its table)."""
    return np.where(np.random.RandomState(seed).randint(0, 10, n) == 0, 0x42, 0x41).astype(np.uint8)


def fp32_bytes(nbytes=4 * 65536, seed=12345):
    """fp32 randn * 0.02 (numpy's, rounded from double: the low mantissa bytes are uniform) -> its bytes."""
    return (np.random.RandomState(seed).randn(nbytes // 4) * 0.02).astype("<f4").view(np.uint8).copy()


def fp32_planes(block=65536):
    """One superblock of fp32_bytes split at width 4: blocks 0 .. 3 are the byte planes, low mantissa first."""
    return pc.split_numpy(fp32_bytes(4 * block), 4, block)


def oracle_streams(oracle, data, block, coder):
    """-> (payload, offsets) of the CPU oracle's block streams."""
    slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=8)
    return oracle.compact(slots, sizes)


def pattern(flags):
    return " ".join("S" if f else "c" for f in flags)


# the CPU oracle's decisions at gain 0 on mixed_bytes(block): S = stored, c = kept
PATTERNS = {
    4096: {0: "S c S c S c", 1: "S c S c S c", 2: "S S S c S S", 3: "S S S S S S"},
    65536: {0: "S c S c S c", 1: "S c S c S c", 2: "S c S c S c", 3: "S c S S S c"},
}
