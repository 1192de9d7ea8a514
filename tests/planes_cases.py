"""What the byte-plane tests share (tests/test_planes_cpu.py, tests/test_gpu_planes.py): the transform of
include/rcx_planes.h restated in numpy, the typed buffers, and the case lists.  Not a test file."""
import numpy as np

WIDTHS = (2, 4, 8)


def _by_superblock(x, width, block, forward):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    out = x.copy()  # (the R % width tail bytes of every superblock keep their places)
    for at in range(0, len(x), width * block):
        m = min(width * block, len(x) - at) // width
        part = x[at: at + m * width]
        out[at: at + m * width] = (part.reshape(m, width).T if forward else part.reshape(width, m).T).reshape(-1)
    return out


def split_numpy(x, width, block):
    """Superblock by superblock (width * block bytes): plane p = byte p of every whole element, planes one after the other."""
    return _by_superblock(x, width, block, True)


def join_numpy(y, width, block):
    return _by_superblock(y, width, block, False)


# ---- the kernel's shapes ---------------------------------------------------------------------------------------------------
BLOCKS = (16, 48, 100, 4096)  # 100: the planes themselves start off 16-byte borders; 48, 100: a superblock is not whole steps
OFFSETS = (0, 1, 3, 8, 15)


def sizes(width, block):
    """n: nothing, below and at one element, around one unit of 16 elements, around one superblock, a ragged fourth."""
    w, wb = width, width * block
    return (0, 1, w - 1, w, 16 * w - 1, 16 * w, 16 * w + 1, wb - 1, wb, wb + 1, wb + w, 3 * wb + 5)


def kernel_cases():
    """(width, block, n, source offset, destination offset): every n at every block and width; the offsets cycle through
    all 25 pairs independently of the shape, so every offset occurs on both sides, with B = 100 too."""
    out, k = [], 0
    for width in WIDTHS:
        for block in BLOCKS:
            for n in sizes(width, block):
                out.append((width, block, n, OFFSETS[k % 5], OFFSETS[(k // 5 + k) % 5]))
                k += 1
    return out


# ---- typed buffers ---------------------------------------------------------------------------------------------------------
def randn_bytes(dtype_name, nbytes=1 << 20, seed=12345):
    """torch.randn(seed) * 0.02 in bf16, fp16 or fp32 -> (its bytes as uint8, the element width)."""
    import torch
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    width = torch.empty(0, dtype=dtype).element_size()
    torch.manual_seed(seed)
    t = (torch.randn(nbytes // width) * 0.02).to(dtype)
    return t.view(torch.uint8).numpy().copy(), width


def index_bytes(nbytes=1 << 20, below=50_000, seed=12345):
    """int64 indices below `below` -> (their bytes, 8): five of an element's eight bytes are zero."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, below, nbytes // 8).astype("<i8").view(np.uint8).copy(), 8


def total_size(oracle, data, block, coder):
    """Bytes of the compacted block streams the reference's coder makes of `data`."""
    _, sizes_ = oracle.encode_blocks(data, block, coder=coder, threads=8)
    return int(sizes_.astype(np.int64).sum())
