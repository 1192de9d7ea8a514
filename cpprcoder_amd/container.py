"""A file container around the many-block coder ("multi-block container"; 8(f) row 3).

The reference has no multi-block format (one stream per file, test/main.cpp:304-364); this is the framing the
block engine needs to be usable on files.  Every block's stream inside is bit-exact what the reference's
AdaptiveRangeEncoder (or RangeEncoder, coder = 1; rANS::encode, coder = 2; rANS::encode_simd, coder = 3) emits
for that block, so a reader with only the reference can decode a container block by block.

Layout (little-endian):
    0   4  magic  b"RCXB"
    4   1  version (1)
    5   1  coder   (0 adaptive, 1 static, 2 rANS one state, 3 rANS eight states: include/rcx.h RCX_CODER_*)
    6   2  flags: bit 0 = the data went through the reference's block sort first (blksort.h: BlkSort::encode, 2 bytes
           more per whole 32 KiB, as test/main.cpp:961-970 does in front of zlib / zstd); other bits 0
    8   4  block size in bytes
    12  8  n, the original size
    20  8  nblocks = ceil(m / block), m = the bytes the coder saw: n, or with bit 0 n + 2 * (n // 32768)
    28  8 * (nblocks + 1)  offsets of the block streams in the payload (offsets[0] = 0, offsets[nblocks] = payload size)
    ..  payload: the block streams back to back

The header functions are plain Python; pack()/unpack() go through the HIP library (there is no CPU coder
here: without librcx.so and a GPU they raise).

unpack_range(blob, start, stop) decodes only the blocks that cover [start, stop), through the item call
(rcx_decode_items: any subset of a set of streams).  It is refused for block-sorted containers, whose bytes are
not in place before the whole inverse transform has run.

The item container holds independent buffers of differing sizes (include/rcx.h, "Item calls"), each coded as the
reference codes a file of those bytes; an item of length 0 has no stream.  Its own magic, so that parse() keeps
rejecting what it does not know:
    0   4  magic  b"RCXI"
    4   1  version (1)
    5   1  coder
    6   2  flags (0)
    8   8  nitems
    16  8 * nitems        the items' lengths
    ..  8 * (nitems + 1)  offsets of the item streams in the payload
    ..  payload: the item streams back to back
"""
import struct

import numpy as np

MAGIC = b"RCXB"
VERSION = 1
FLAG_BLKSORT = 1
_FIXED = struct.Struct("<4sBBHIQQ")
ITEM_MAGIC = b"RCXI"
ITEM_VERSION = 1
_ITEM_FIXED = struct.Struct("<4sBBHQ")
MAX_ITEM = (1 << 24) - 256  # RCX_MAX_BLOCK


def coded_size(n: int, flags: int) -> int:
    """What the entropy coder is handed for n original bytes (blksort.h:426-431 if block-sorted)."""
    return n + 2 * (n // 32768) if flags & FLAG_BLKSORT else n


class ContainerError(ValueError):
    pass


def header_bytes(coder: int, block: int, n: int, offsets, flags: int = 0) -> bytes:
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    nblocks = len(offsets) - 1
    if nblocks != (coded_size(n, flags) + block - 1) // block:
        raise ContainerError("offsets do not match n and the block size")
    return _FIXED.pack(MAGIC, VERSION, coder, flags, block, n, nblocks) + offsets.tobytes()


def parse(blob):
    """-> dict(coder, flags, block, n, nblocks, offsets uint64[nblocks+1], payload uint8 view)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, block, n, nblocks = _FIXED.unpack(bytes(buf[: _FIXED.size]))
    if magic != MAGIC:
        raise ContainerError("not an RCXB container")
    if version != VERSION or coder not in (0, 1, 2, 3) or flags & ~FLAG_BLKSORT:
        raise ContainerError("unsupported container version, coder or flags")
    if block < 16 or block > (1 << 24) - 256 or nblocks != (coded_size(n, flags) + block - 1) // block:
        raise ContainerError("inconsistent header")
    end = _FIXED.size + 8 * (nblocks + 1)
    if len(buf) < end:
        raise ContainerError("truncated offset table")
    offsets = np.frombuffer(bytes(buf[_FIXED.size:end]), dtype="<u8").astype(np.uint64)
    if offsets[0] != 0 or np.any(np.diff(offsets.astype(np.int64)) < 0) or end + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    return {"coder": coder, "flags": flags, "block": block, "n": n, "nblocks": nblocks, "offsets": offsets, "payload": buf[end:]}


def pack(data, block: int = 65536, coder: int = 0, ctx=None, blksort: bool = False) -> bytes:
    from . import rcx
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        src = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        flags = FLAG_BLKSORT if blksort else 0
        if len(src) == 0:
            return header_bytes(coder, block, 0, np.zeros(1, np.uint64), flags)
        payload, offsets = ctx.encode_blocks(ctx.bwt_encode(src) if blksort else src, block, coder=coder)
        return header_bytes(coder, block, len(src), offsets, flags) + payload.tobytes()
    finally:
        if own:
            ctx.close()


def unpack(blob, ctx=None) -> bytes:
    from . import rcx
    c = parse(blob)
    if c["n"] == 0:
        return b""
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        m = coded_size(c["n"], c["flags"])
        out = ctx.decode_blocks(c["payload"], c["offsets"], c["block"], capacity=m, coder=c["coder"])
        if len(out) != m:
            raise ContainerError("decoded size differs from the header")
        if c["flags"] & FLAG_BLKSORT:
            out = ctx.bwt_decode(out)
        return out.tobytes()
    finally:
        if own:
            ctx.close()


def unpack_range(blob, start: int, stop: int, ctx=None) -> bytes:
    """The bytes [start, stop) of the original, decoding only the blocks that cover them."""
    from . import rcx
    c = parse(blob)
    if c["flags"] & FLAG_BLKSORT:
        raise ContainerError("a block-sorted container has no byte ranges: unpack() it")
    if not 0 <= start <= stop <= c["n"]:
        raise ContainerError("range outside the data")
    if start == stop:
        return b""
    block, n = c["block"], c["n"]
    first, last = start // block, (stop - 1) // block
    pick = np.arange(first, last + 1, dtype=np.uint64)
    lengths = np.full(c["nblocks"], block, dtype=np.uint64)
    lengths[-1] = n - (c["nblocks"] - 1) * block
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        parts = ctx.decode_items(c["payload"], c["offsets"], lengths, pick=pick, coder=c["coder"])
    finally:
        if own:
            ctx.close()
    out = np.concatenate(parts)
    return out[start - first * block: stop - first * block].tobytes()


def item_header_bytes(coder: int, lengths, offsets) -> bytes:
    lengths = np.ascontiguousarray(lengths, dtype="<u8")
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    if len(offsets) != len(lengths) + 1:
        raise ContainerError("offsets do not match the number of items")
    if len(lengths) and int(lengths.max()) > MAX_ITEM:
        raise ContainerError("an item is longer than the coder takes")
    return _ITEM_FIXED.pack(ITEM_MAGIC, ITEM_VERSION, coder, 0, len(lengths)) + lengths.tobytes() + offsets.tobytes()


def parse_items(blob):
    """-> dict(coder, nitems, lengths uint64[nitems], offsets uint64[nitems+1], payload uint8 view)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _ITEM_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, nitems = _ITEM_FIXED.unpack(bytes(buf[: _ITEM_FIXED.size]))
    if magic != ITEM_MAGIC:
        raise ContainerError("not an RCXI container")
    if version != ITEM_VERSION or coder not in (0, 1, 2, 3) or flags:
        raise ContainerError("unsupported container version, coder or flags")
    mid = _ITEM_FIXED.size + 8 * nitems
    end = mid + 8 * (nitems + 1)
    if nitems > len(buf) or len(buf) < end:
        raise ContainerError("truncated tables")
    lengths = np.frombuffer(bytes(buf[_ITEM_FIXED.size:mid]), dtype="<u8").astype(np.uint64)
    offsets = np.frombuffer(bytes(buf[mid:end]), dtype="<u8").astype(np.uint64)
    if nitems and int(lengths.max()) > MAX_ITEM:
        raise ContainerError("an item is longer than the coder takes")
    sizes = np.diff(offsets.astype(np.int64))
    if offsets[0] != 0 or np.any(sizes < 0) or end + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    if np.any((lengths == 0) != (sizes == 0)):
        raise ContainerError("an item of length 0 has no stream, and only such an item")
    return {"coder": coder, "nitems": nitems, "lengths": lengths, "offsets": offsets, "payload": buf[end:]}


def pack_items(items, coder: int = 0, ctx=None) -> bytes:
    """items: a list of buffers -> an RCXI container."""
    from . import rcx
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        parts = [np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if not isinstance(x, np.ndarray) else x, dtype=np.uint8) for x in items]
        payload, offsets = ctx.encode_items(parts, coder=coder)
        return item_header_bytes(coder, [len(x) for x in parts], offsets) + payload.tobytes()
    finally:
        if own:
            ctx.close()


def unpack_items(blob, pick=None, ctx=None) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None); picks may repeat."""
    from . import rcx
    c = parse_items(blob)
    if pick is not None and any(not 0 <= int(k) < c["nitems"] for k in pick):
        raise ContainerError("no such item")
    if c["nitems"] == 0 or (pick is not None and len(pick) == 0):
        return []
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        return [x.tobytes() for x in ctx.decode_items(c["payload"], c["offsets"], c["lengths"], pick=pick, coder=c["coder"])]
    finally:
        if own:
            ctx.close()
