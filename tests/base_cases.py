"""What the base-residual tests share (tests/test_base_cpu.py, tests/test_gpu_base.py): the case lists, the data kinds, edge
pairs and the checkpoint recipe.  The transform's numpy statement is the package's own (cpprcoder_amd/base.py: split_numpy,
join_numpy).  Not a test file."""
import numpy as np

import planes_cases as pc
from cpprcoder_amd import base

WIDTHS = base.WIDTHS
OPS = base.OPS
NAMES = {base.XOR: "xor", base.SUB: "sub", base.SUBZZ: "subzz"}

# ---- the kernel's shapes ---------------------------------------------------------------------------------------------------
# 16, 48, 100: a superblock of less than a step, planes off 16-byte borders (100), rest elements behind the units (100);
# 4096: whole steps; 4112: a unit more than that.
BLOCKS = (16, 48, 100, 4096, 4112)
OFFSETS = pc.OFFSETS
ROWS = {1: 8, 2: 4, 4: 2, 8: 1}  # RCX_BASE_U4 / (2 * width): rows of 256 units a workgroup takes at a time (csrc/rcx_base.hpp)


def step_bytes(width):
    """The source bytes of one step of a workgroup of rcx_base_k: while a whole step is left the kernel takes the path without
    bounds tests (GUARD = false), the last step takes the one with them."""
    return ROWS[width] * 256 * 16 * width


def sizes(width, block):
    """n: planes_cases.sizes (nothing, around one element, one unit, one superblock, a ragged fourth) -- for width 1 the same
    list, where an element is a byte and a superblock a block -- and the kernel's own border: exactly one step, and one step, a
    unit, an element and a byte more, so that the path without bounds tests runs once and the one with them behind it."""
    step = step_bytes(width)
    return tuple(dict.fromkeys(pc.sizes(width, block) + (step, step + 17 * width + 1)))


def kernel_cases():
    """(width, block, n, source offset, base offset, destination offset): every n at every block and width; the three offsets
    cycle through (0, 1, 3, 8, 15) independently of the shape and of one another."""
    out, k = [], 0
    for width in WIDTHS:
        for block in BLOCKS:
            for n in sizes(width, block):
                out.append((width, block, n, OFFSETS[k % 5], OFFSETS[(k // 5 + k) % 5], OFFSETS[(k // 25 + 2 * k) % 5]))
                k += 1
    return out


KINDS = ("random", "equal", "minus_one", "straddle")  # straddle: width 8 only


def kernel_data(kind, width, nbytes, noise):
    """-> (source, base), nbytes each.  random: independent random bytes, every difference wraps.  equal: the source is the base,
    every residual 0.  minus_one: source element = base element - 1, the borrow runs through every byte and the zigzag is 1.
    straddle (width 8): base elements 2^32 + k, source elements 2^32 - 1 - k and the other way round in turn: the pair lies on
    both sides of the border of the words."""
    ref = np.array(noise[:nbytes])
    if kind == "random":
        return np.array(noise[nbytes + 5: 2 * nbytes + 5]), ref
    if kind == "equal":
        return ref.copy(), ref
    count = -(-nbytes // width)
    dtype = np.dtype(f"<u{width}")
    if kind == "minus_one":
        b = np.zeros(count * width, np.uint8)
        b[:nbytes] = ref
        e = (b.view(dtype) - dtype.type(1)).astype(dtype)
        return e.view(np.uint8)[:nbytes].copy(), ref
    assert kind == "straddle" and width == 8
    k = np.arange(count, dtype=np.uint64)
    above, below = np.uint64(1 << 32) + k, np.uint64((1 << 32) - 1) - k
    e, b = np.where(k & np.uint64(1), above, below).astype("<u8"), np.where(k & np.uint64(1), below, above).astype("<u8")
    return e.view(np.uint8)[:nbytes].copy(), b.view(np.uint8)[:nbytes].copy()


def edge_units(width):
    """Units of 16 elements for the host program, source and base -> (e, b) uint8 [units, 16 * width]: elements equal to the
    base; base - 1 and base + 1 (the borrow, the carry, through every byte); the most negative difference, 2^(8 * width - 1),
    and its neighbours; all ones against zero and the other way; for width 8 pairs on both sides of 2^32; random ones."""
    bits = 8 * width
    mask, dtype = (1 << bits) - 1, np.dtype(f"<u{width}")
    rs = np.random.RandomState(90 + width)
    rand = [int.from_bytes(rs.bytes(width), "little") for _ in range(16)]
    half = 1 << (bits - 1)
    pairs = [(v, v) for v in rand[:4]] + [((v - 1) & mask, v) for v in (0, 1, half, mask, 1 << (bits // 2)) + tuple(rand[4:8])]
    pairs += [((v + 1) & mask, v) for v in (0, mask, half - 1, (1 << (bits // 2)) - 1) + tuple(rand[8:10])]
    pairs += [((v + half) & mask, v) for v in (0, 1, mask, rand[10])] + [((v + half - 1) & mask, v) for v in (0, rand[11])]
    pairs += [((v + half + 1) & mask, v) for v in (0, rand[12])] + [(mask, 0), (0, mask), (0, 0), (mask, mask)]
    if width == 8:
        pairs += [((1 << 32) - 1, 1 << 32), (1 << 32, (1 << 32) - 1), ((1 << 32) + 5, (1 << 32) - 7), ((1 << 32) - 7, (1 << 32) + 5)]
    pairs += [(int.from_bytes(rs.bytes(width), "little"), int.from_bytes(rs.bytes(width), "little")) for _ in range(16 * 24)]
    while len(pairs) % 16:
        pairs.append(pairs[len(pairs) % 7])
    e = np.array([p[0] for p in pairs], np.uint64).astype(dtype).view(np.uint8).reshape(-1, 16 * width)
    b = np.array([p[1] for p in pairs], np.uint64).astype(dtype).view(np.uint8).reshape(-1, 16 * width)
    return e, b


# ---- the data the stage is for -----------------------------------------------------------------------------------------------
def bf16_bytes(a):
    """float32 -> the bytes of its bf16 rounding, round-to-nearest-even on the fp32 bits."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype("<u2").view(np.uint8)


def checkpoint_pair(count=1 << 20, step=1e-4):
    """-> (w2, w, unrelated), bf16 bytes: weights randn * 0.02, the same moved by randn * step, and an independent randn * 0.02."""
    rng = np.random.default_rng(1)
    w = (rng.standard_normal(count) * 0.02).astype(np.float32)
    w2 = (w + rng.standard_normal(count) * step).astype(np.float32)
    other = (rng.standard_normal(count) * 0.02).astype(np.float32)
    return bf16_bytes(w2), bf16_bytes(w), bf16_bytes(other)


def counter_pair(count=1 << 17):
    """-> (now, before), uint64 bytes: counters below 2^40 and the same plus randint(0, 50)."""
    rng = np.random.default_rng(2)
    before = rng.integers(0, 1 << 40, count, dtype=np.uint64)
    now = before + rng.integers(0, 50, count, dtype=np.uint64)
    return now.astype("<u8").view(np.uint8), before.astype("<u8").view(np.uint8)
