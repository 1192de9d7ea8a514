"""What the predictor tests share (tests/test_predict_cpu.py, tests/test_gpu_predict.py): the transform of
include/rcx_predict.h restated in numpy, the integer buffers it is for, and the case lists.  Not a test file."""
import numpy as np

import planes_cases as pc

WIDTHS = pc.WIDTHS
NONE, DELTA, ZIGZAG = 0, 1, 2
PREDS = (DELTA, ZIGZAG)
NAMES = {DELTA: "delta", ZIGZAG: "zigzag"}


def zigzag(d):
    """d: an unsigned array -> (d << 1) ^ (0 - (d >> (bits - 1))), logical shifts, modulo 2^bits."""
    bits = d.dtype.type(8 * d.dtype.itemsize)
    one = d.dtype.type(1)
    return (d << one) ^ (d.dtype.type(0) - (d >> (bits - one)))


def unzigzag(z):
    one = z.dtype.type(1)
    return (z >> one) ^ (z.dtype.type(0) - (z & one))


def _by_superblock(x, width, block, pred, forward):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    out = x.copy()  # (the R % width tail bytes of every superblock keep their values and places)
    if pred == NONE:
        return out
    dtype = np.dtype(f"<u{width}")
    for at in range(0, len(x), width * block):
        m = min(width * block, len(x) - at) // width
        if m == 0:
            continue
        e = x[at: at + m * width].view(dtype)  # unsigned: numpy wraps modulo 2^(8 * width)
        if forward:
            d = e.copy()
            d[1:] = e[1:] - e[:-1]  # np.diff, with d_0 = e_0: the predictor restarts here
            r = zigzag(d) if pred == ZIGZAG else d
        else:
            r = np.cumsum(unzigzag(e) if pred == ZIGZAG else e, dtype=dtype)
        out[at: at + m * width] = r.astype(dtype).view(np.uint8)
    return out


def predict_numpy(x, width, block, pred):
    """Superblock by superblock (width * block bytes): every whole element becomes its difference to the one in front."""
    return _by_superblock(x, width, block, pred, True)


def unpredict_numpy(y, width, block, pred):
    return _by_superblock(y, width, block, pred, False)


def split_numpy(x, width, block, pred):
    """What rcx_predict_split makes: the planes of the predicted elements."""
    return pc.split_numpy(predict_numpy(x, width, block, pred), width, block)


def join_numpy(y, width, block, pred):
    return unpredict_numpy(pc.join_numpy(y, width, block), width, block, pred)


# ---- the kernels' shapes -------------------------------------------------------------------------------------------------
# The inverse kernel's tile is one wave of 64 units = 1024 elements; a superblock is walked tile by tile.
#   16, 48, 100     less than a unit row, off 16-byte borders; tiles with idle lanes
#   1024, 1040      one tile (a wave's 64 units), and one unit more
#   3072, 5120      three and five tiles: the inverse takes whole rows two a turn, an odd count leaves the other remainder
#   4096, 4112      four tiles, and one unit more
#   12304           twelve tiles and a unit: the carry crosses tiles
BLOCKS = (16, 48, 100, 1024, 1040, 3072, 4096, 4112, 5120, 12304)
OFFSETS = pc.OFFSETS
KINDS = ("random", "minus_k", "ramp")  # ramp: width 8 only


def kernel_cases():
    """(width, block, n, source offset, destination offset): every n of planes_cases.sizes at every block and width; the
    offsets cycle through all 25 pairs independently of the shape."""
    out, k = [], 0
    for width in WIDTHS:
        for block in BLOCKS:
            for n in pc.sizes(width, block):
                out.append((width, block, n, OFFSETS[k % 5], OFFSETS[(k // 5 + k) % 5]))
                k += 1
    return out


def kernel_data(kind, width, nbytes, noise):
    """nbytes bytes of elements: `random` -- every sum wraps; `minus_k` -- the elements -k: every byte of every difference
    is 0xFF and the carry runs through every byte; `ramp` (width 8) -- e_k = 2^32 - 8 + k, across the border of the words."""
    if kind == "random":
        return noise[:nbytes]
    count = -(-nbytes // width)
    k = np.arange(count, dtype=np.uint64)
    if kind == "minus_k":
        e = (np.uint64(0) - k).astype(f"<u{width}")
    else:
        assert kind == "ramp" and width == 8
        e = (np.uint64((1 << 32) - 8) + k).astype("<u8")
    return e.view(np.uint8)[:nbytes].copy()


# ---- the integer buffers the predictor is for -------------------------------------------------------
def integer_bytes(name, nbytes=1 << 20, seed=12345):
    """-> (the bytes, the element width); each from its own RandomState(seed)."""
    rs = np.random.RandomState(seed)
    if name == "sorted_keys":  # sorted 64-bit keys below 10^9
        return np.sort(rs.randint(0, 10 ** 9, nbytes // 8)).astype("<i8").view(np.uint8).copy(), 8
    if name == "csr_offsets":  # row offsets of a sparse matrix with up to 63 entries a row
        return np.cumsum(rs.randint(0, 64, nbytes // 8)).astype("<i8").view(np.uint8).copy(), 8
    if name == "random_walk":  # steps of both signs
        return np.cumsum(rs.randint(-100, 101, nbytes // 4)).astype("<i4").view(np.uint8).copy(), 4
    assert name == "signal"    # a sampled sine with noise
    count = nbytes // 2
    return (np.sin(np.arange(count) / 50.0) * 8000 + rs.randint(-20, 21, count)).astype("<i2").view(np.uint8).copy(), 2


def looping_cases(waves):
    """(width, block, n) with more superblocks than the inverse kernel's grid has waves (`waves` = 32 a compute unit; twice as
    many and more where a superblock is small), so that the grid loops and a wave owns several superblocks: superblocks of one row with idle lanes, of two rows,
    and of four rows (three whole ones: the two-a-turn loop runs behind a row that was loaded ahead); the ragged last
    superblock with fewer than 16 elements (no unit: nothing to load ahead), and with a unit, rest elements and tail bytes."""
    count, fewer = 2 * waves + 37, waves + 37
    return ((8, 16, count * 8 * 16 + 8 * 5 + 3),        # last: 5 elements and 3 bytes
            (4, 48, count * 4 * 48 + 4 * 21 + 1),        # last: a unit, 5 rest elements, a byte
            (2, 1040, fewer * 2 * 1040 + 2 * 7 + 1),     # two rows a superblock; last: 7 elements and a byte
            (2, 3088, fewer * 2 * 3088 + 2 * 1500 + 1))  # four rows a superblock, three of them whole; last: two rows


INTEGER_BUFFERS = ("sorted_keys", "csr_offsets", "random_walk", "signal")
