"""What the statistics tests share (tests/test_stats_cpu.py, tests/test_gpu_stats.py): per-block counts and costs of
include/rcx_stats.h restated with np.bincount and stats.cost_numpy, the eight typed buffers the rule of
pack_typed(predict="auto") is held to with the pick expected of it, and the shapes and data of the kernel tests.  Not a test file."""
import numpy as np

import planes_cases as pc
import predict_cases as pr
from cpprcoder_amd import stats

SHORT = 1024  # csrc/rcx_stats.hpp RCX_STATS_SHORT: an entry of at most this many bytes is counted by one wave


# ---- the tables in numpy -----------------------------------------------------------------------------------------------------
def hist_items(x, offs):
    """-> uint32 [nitems, 256]: np.bincount of every item x[offs[i] : offs[i + 1]]."""
    out = np.zeros((len(offs) - 1, 256), np.uint32)
    for i in range(len(offs) - 1):
        out[i] = np.bincount(x[int(offs[i]): int(offs[i + 1])], minlength=256)
    return out


def hist_blocks(x, block):
    n = len(x)
    whole = n // block
    out = np.zeros((-(-n // block), 256), np.uint32)
    if whole:  # all whole blocks in one bincount: block b's symbol c is bin b * 256 + c
        keys = x[: whole * block].astype(np.int64) + 256 * np.repeat(np.arange(whole, dtype=np.int64), block)
        out[:whole] = np.bincount(keys, minlength=256 * whole).reshape(whole, 256)
    if n % block:
        out[whole] = np.bincount(x[whole * block:], minlength=256)
    return out


def cost_blocks(x, block):
    return stats.cost_numpy(hist_blocks(x, block))


def cost_bytes(units):
    """A cost (bits times 65536) in bytes, to the nearest."""
    return (int(units) + 4 * stats.UNIT) // (8 * stats.UNIT)


# ---- the typed buffers of the rule -----------------------------------------------------------------------------------------
# name -> the pick the issue's table and DESIGN.md section 13 state
PICKS = {"sorted_keys": "delta", "csr_offsets": "delta", "random_walk": "zigzag", "signal": "delta",
         "indices": None, "bf16": None, "fp32": None, "uniform": None}


def typed_bytes(name):
    """-> (1 MiB of bytes, the element width)"""
    if name in pr.INTEGER_BUFFERS:
        return pr.integer_bytes(name)
    if name == "indices":
        return pc.index_bytes()
    if name in ("bf16", "fp32"):
        return pc.randn_bytes(name)
    assert name == "uniform"
    return np.random.RandomState(12345).randint(0, 256, 1 << 20, dtype=np.uint8), 4


def split_costs(x, width, block):
    """(C_none, C_delta, C_zigzag): the summed block costs of the split text under each predictor, as Python integers."""
    return tuple(int(cost_blocks(pr.split_numpy(x, width, block, pred), block).sum(dtype=np.uint64)) for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG))


# ---- the kernel's shapes and data ------------------------------------------------------------------------------------------
# 16, 100         one wave an entry (at most SHORT bytes), 100 off the 16-byte pieces
# 1024, 1040      the last block size a wave takes alone and the first the workgroup takes
# 4096, 4112      one row of the workgroup's 16-byte loads, and one piece more
# 65536           four rows in flight, four times
BLOCKS = (16, 100, 1024, 1040, 4096, 4112, 65536)
OFFSETS = pc.OFFSETS
KINDS = ("uniform", "one_byte", "two_values", "each_once")


def sizes(block):
    """n: a byte, one block less a byte, one, two and a byte, three and a ragged tail."""
    return (1, block - 1, block, 2 * block + 1, 3 * block + block // 3 + 5)


def data(kind, n, noise):
    if kind == "uniform":
        return noise[:n]
    if kind == "one_byte":
        return np.full(n, 0xA7, np.uint8)
    if kind == "two_values":
        return np.where(np.arange(n) % 2 == 0, 0x00, 0xFF).astype(np.uint8)
    assert kind == "each_once"  # every value exactly once in every 256
    return (np.arange(n) * 7 + 3).astype(np.uint8)
