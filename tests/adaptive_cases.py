"""Inputs for the adaptive coder's kernels that several tests share: bursts of very improbable symbols (the decoder's
synchronous ring refill, the encoder's drain), blocks of one value (the largest counts and sums), and the block lengths that
stand on the boundaries between the quad decoder's three loops.  Pure: numpy and the generators only; expected bytes always
come from the oracle.  tests/crafted_cases.py lists every family here for the comparison with the reference build, and
tests/test_oracle_crafted.py pins every builder's bytes.
"""
import numpy as np

from cpprcoder_amd import workloads

# ---- the quad decoder's pass of 64 symbols (tests/test_gpu_dec_pass64.py) -------------------------------------------------
PASS_BLOCK = 4096
ALL_THREE = 64 * 5 + 16 * 3 + 7  # five passes, three groups, seven symbols one by one
PASS_LENGTHS = (48, 64, 80, 112, 128, 129, 191, 192, ALL_THREE)
PASS_BURST_GROUPS = (1, 2, 3)


def pass_burst_blocks(group):
    """16 blocks of 4 KiB: after some 3000 equal bytes every other value costs about 12 bits, 6 dwords per 16 symbols where
    the top-up supplies 4, so the input ring runs low and the synchronous refill runs, again and again every few groups for
    the 32 groups the burst lasts.  The burst begins two groups in front of group `group` of a pass, in a pass of its own
    in every other block."""
    rs = np.random.RandomState(8600 + group)
    blocks = []
    for b in range(16):
        fill = (65, 0, 255, 128)[b % 4]
        x = np.full(PASS_BLOCK, fill, np.uint8)
        others = np.array([v for v in range(256) if v != fill], np.uint8)
        at = 3072 + 64 * (b % 8) + 16 * group - 32
        burst = np.concatenate([rs.permutation(others), rs.permutation(others)])[: PASS_BLOCK - at]
        x[at: at + len(burst)] = burst
        blocks.append(x)
    return blocks


# ---- bursts behind 2^20 equal bytes (tests/test_gpu_parity.py) -----------------------------------------------------------
LONG_BURST_BLOCK = 1 << 20
LONG_BURSTS = ((65, 1), (0, 2), (255, 3))  # (the repeated byte, seed)


def long_burst_block(fill, seed):
    """After ~2^20 equal bytes every other byte value costs 20 bits: 2.5 output bytes per symbol for a while; and once
    early, at 13 bits per symbol."""
    block = LONG_BURST_BLOCK
    rs = np.random.RandomState(seed)
    d = np.full(block, fill, np.uint8)
    others = np.array([v for v in range(256) if v != fill], np.uint8)
    tail = np.concatenate([rs.permutation(others) for _ in range(24)])
    d[block - len(tail):] = tail
    d[5000:5000 + 255] = rs.permutation(others)  # and once early, at 13 bits per symbol
    return d


def long_bursts():
    """The three burst blocks and one block of zipf bytes, in one buffer."""
    return np.concatenate([long_burst_block(fill, seed) for fill, seed in LONG_BURSTS] + [workloads.zipf(LONG_BURST_BLOCK, 4)])


# ---- blocks of one value ----------------------------------------------------------------------------------------------------
ONE_VALUE_N = 1 << 18
ONE_VALUE_BYTES = (0, 255)


def one_value_block(byte, n=ONE_VALUE_N):
    """n symbols of one value: its count -- and every bound above it -- grows to n while t falls to range / n."""
    return np.full(n, byte, np.uint8)


LEVEL3_CASES = ("all 0", "all 255", "0 then 255")


def level3_block(case):
    """One block of 65536 symbols (tests/test_gpu_enc_seven_waves.py).  Of symbol 0 alone: all three level-3 sums grow with
    every symbol, to 65536 + 192.  Of symbol 255 alone: the sum below the last quarter is handed over with every symbol.
    Of symbol 0 with a 255 now and then, and as the last symbol: the largest sums there can be, up to 192 + 65535."""
    data = np.full(65536, 255 if case == "all 255" else 0, np.uint8)
    if case == "0 then 255":
        data[np.random.RandomState(3).randint(0, 65536, 300)] = 255
        data[-1] = 255
    return data
