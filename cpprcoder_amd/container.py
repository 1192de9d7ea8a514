"""A file container around the many-block coder ("multi-block container"; 8(f) row 3).

The reference has no multi-block format (one stream per file, test/main.cpp:304-364); this is the framing the
block engine needs to be usable on files.  Every block's stream inside is bit-exact what the reference's
AdaptiveRangeEncoder (or RangeEncoder, coder = 1; rANS::encode, coder = 2; rANS::encode_simd, coder = 3) emits
for that block, so a reader with only the reference can decode a container block by block.

Layout (little-endian):
    0   4  magic  b"RCXB"
    4   1  version (1; 2 with checksums)
    5   1  coder   (0 adaptive, 1 static, 2 rANS one state, 3 rANS eight states: include/rcx.h RCX_CODER_*)
    6   2  flags: bit 0 = the data went through the reference's block sort first (blksort.h: BlkSort::encode, 2 bytes
           more per whole 32 KiB, as test/main.cpp:961-970 does in front of zlib / zstd); bit 1 = checksums (version 2,
           and only there); other bits 0
    8   4  block size in bytes
    12  8  n, the original size
    20  8  nblocks = ceil(m / block), m = the bytes the coder saw: n, or with bit 0 n + 2 * (n // 32768)
    28  8 * (nblocks + 1)  offsets of the block streams in the payload (offsets[0] = 0, offsets[nblocks] = payload size)
    ..  version 2: 4 * nblocks  the CRC-32 (zlib's crc32, u32 LE) of each block of the bytes the coder saw -- with bit 0 the
        block-sorted text -- so that a block can be checked on its own, by unpack_range() too
    ..  payload: the block streams back to back

Checksums are opt-in (pack(..., checksum=True)): without them a container is byte for byte what it always was, version
1.  The decoders cannot tell that a damaged payload came back wrong (include/rcx.h, "Damaged streams": it still decodes to
some bytes); with checksums unpack(), unpack_range() and unpack_items() compare what they decoded, on the GPU, before
they hand it back, and raise ChecksumError naming the first bad block or item (verify=False skips that).  The checked
paths upload once and use the device calls (encode + CRC, decode + verify): they give up the overlap of copies and
kernels that the host-buffer calls have.

The header functions are plain Python; pack()/unpack() go through the HIP library (there is no CPU coder
here: without librcx.so and a GPU they raise).

unpack_range(blob, start, stop) decodes only the blocks that cover [start, stop), through the item call
(rcx_decode_items: any subset of a set of streams).  It is refused for block-sorted containers, whose bytes are
not in place before the whole inverse transform has run.

The item container holds independent buffers of differing sizes (include/rcx.h, "Item calls"), each coded as the
reference codes a file of those bytes; an item of length 0 has no stream.  Its own magic, so that parse() keeps
rejecting what it does not know:
    0   4  magic  b"RCXI"
    4   1  version (1; 2 with checksums)
    5   1  coder
    6   2  flags (0; version 2: bit 1 = checksums)
    8   8  nitems
    16  8 * nitems        the items' lengths
    ..  8 * (nitems + 1)  offsets of the item streams in the payload
    ..  version 2: 4 * nitems  the CRC-32 of each item (u32 LE; 0 for an empty one)
    ..  payload: the item streams back to back

The typed container holds one buffer of 2-, 4- or 8-byte elements (bf16 / fp16 / fp32 values, int32 / int64 indices) that
went through the byte-plane filter (include/rcx_planes.h; cpprcoder_amd/planes.py) in front of the coder: within a
superblock of width * block bytes, block s * width + p holds byte p of every element, so each byte position gets a model
of its own.  A third magic, so that parse() and parse_items() keep refusing what they do not know:
    0   4  magic  b"RCXT"
    4   1  version (1; 2 with a predictor)
    5   1  coder
    6   2  flags: bit 1 = checksums (FLAG_CRC32); every other bit 0
    8   4  block size in bytes
    12  8  n
    20  8  nblocks = ceil(n / block)
    28  1  width: bytes per element (2, 4 or 8)
    29  1  version 2: the predictor in front of the filter (include/rcx_predict.h: 1 delta, 2 delta + zigzag); version 1: zero
    30  6  zero
    36  8 * (nblocks + 1)  offsets of the block streams in the payload
    ..  with bit 1: 4 * nblocks  the CRC-32 of each block of the SPLIT text (what the coder saw, as with the block sort;
        with a predictor the predicted and split text)
    ..  payload
unpack_typed_range(blob, start, stop) decodes the blocks of the superblocks that cover [start, stop) and joins that span
as a buffer of its own: the transform of a span from one superblock border to another, or to n, is the transform of the
span taken alone.  A predictor (pack_typed(..., predict="delta" | "zigzag"): for integers whose differences are small) is
opt-in and restarts in every superblock, so all of that holds with it; without one a container is byte for byte version 1.

Stored blocks (pack(..., stored=True | fraction), pack_typed(..., stored=...); include/rcx_stored.h, cpprcoder_amd/stored.py): a
block whose stream did not shrink -- coded_b + floor(len_b * gain / 65536) >= len_b, gain = 0 for True, min(65535, int(g * 65536))
for a fraction 0 <= g < 1 -- is kept as its len_b raw bytes and decoded by copy, so a payload never exceeds what the coder
saw.  Such a container is version 3 of either layout, and flag bit 2 (FLAG_STORED) is set; the two only ever appear together:
    RCXB version 3: the fixed part as above, flags bit 2 set (bits 0 and 1 as above); offsets; the bitmap; with bit 1 the CRC
        table; payload
    RCXT version 3: the fixed part as above, flags bit 2 set (bit 1 as above), byte 29 = the predictor, 0, 1 or 2; offsets;
        the bitmap; with bit 1 the CRC table; payload
    the bitmap: ceil(nblocks / 8) bytes, block b is bit b & 7 of byte b >> 3, padding bits zero, at least one bit set; a
        stored block's two offsets are len_b apart
The CRC stays the CRC of what the coder saw.  If no block ends up stored the container is, byte for byte, the one written
without the option.  With the option the pack path is the device path of the checked containers: one upload, encode, mix
(and CRC), one download.  An item container has no stored items.

pack_typed(..., predict="auto") measures instead of asking (include/rcx_stats.h; cpprcoder_amd/stats.py).  For each of none,
delta and zigzag the split text's order-0 cost is C_p = the sum of the blocks' costs -- what an order-0 coder with one model a
block will make of it, to within a few percent.  The rule (pick_predictor): a predictor is a candidate only if it earns at
least 1/64, 64 * C_p < 63 * C_none; the cheaper candidate is taken, delta on a tie; without a candidate, none.  The margin
keeps data that no predictor helps on version 1: uniform bytes at 4 KiB blocks would otherwise take delta for 0.002 %.  The
container is byte for byte what predict=<the choice> writes, and nothing in it records that the choice was measured.

The typed item container holds many buffers of differing sizes, each with an element width (1, 2, 4 or 8) and a predictor
of its own (include/rcx_typed_items.h; cpprcoder_amd/typed_items.py): typed item i is transformed as one superblock of
m_i = len_i // w_i elements, and its w_i planes -- the last one with the len_i % w_i tail bytes -- are the coder's items, the
SUB-ITEMS, nsub = the sum of the widths; a sub-item of length 0 has no stream.  A fourth magic:
    0   4  magic  b"RCXJ"
    4   1  version (1)
    5   1  coder
    6   2  flags: bit 1 = checksums (FLAG_CRC32); every other bit 0
    8   8  nitems
    16  8  nsub
    24  8  dlen, the bytes of the directory
    32  8 * nitems      the items' lengths
    ..  nitems          their widths
    ..  nitems          their predictors (include/rcx_predict.h: 0 none, 1 delta, 2 delta + zigzag; 0 with width 1)
    ..  8 * (nsub + 1)  offsets of the sub-item streams in the payload
    ..  with bit 1: 4 * nsub  the CRC-32 of each sub-item of the SPLIT text (0 for an empty one)
    ..  dlen            the directory: the caller's bytes, carried and not interpreted (may be empty)
    ..  payload: the sub-item streams back to back
unpack_typed_items(blob, pick) decodes the picked items' sub-items and no others, verifies those, and joins them as a call of
its own with re-based offsets: every item is a superblock of its own, so any subset is exact.  predict="auto" decides PER
ITEM with pick_predictor on the sum of its sub-items' order-0 costs under the three candidates.  There are no stored
sub-items and no command-line subcommand.  pack_tensors / unpack_tensors put tensors with names on top of it and nothing
else: every tensor is cut into typed items of element_size * block bytes -- its superblocks, so its sub-items are the blocks
pack_typed would code -- and the directory is JSON: a list of {"name", "dtype" (torch's name), "shape", "first", "count"}.
"""
import struct

import numpy as np

MAGIC = b"RCXB"
VERSION = 1
VERSION_CRC = 2  # the same layout + the CRC table; always with FLAG_CRC32
VERSION_STORED = 3  # + the bitmap of the stored blocks behind the offsets; always with FLAG_STORED (RCXB and RCXT)
FLAG_BLKSORT = 1
FLAG_CRC32 = 2
FLAG_STORED = 4
_FIXED = struct.Struct("<4sBBHIQQ")
ITEM_MAGIC = b"RCXI"
ITEM_VERSION = 1
_ITEM_FIXED = struct.Struct("<4sBBHQ")
MAX_ITEM = (1 << 24) - 256  # RCX_MAX_BLOCK
TYPED_MAGIC = b"RCXT"
TYPED_VERSION = 1
TYPED_VERSION_PRED = 2  # the same layout + the predictor at byte 29; only with a predictor
TYPED_VERSION_STORED = VERSION_STORED  # + the bitmap; byte 29 names the predictor, none included
PREDICTORS = {None: 0, "delta": 1, "zigzag": 2}  # include/rcx_predict.h: RCX_PRED_*
AUTO = "auto"  # pack_typed(predict=AUTO): measured, see pick_predictor; never in a container
_TYPED_FIXED = struct.Struct("<4sBBHIQQB7s")
WIDTHS = (2, 4, 8)


def coded_size(n: int, flags: int) -> int:
    """What the entropy coder is handed for n original bytes (blksort.h:426-431 if block-sorted)."""
    return n + 2 * (n // 32768) if flags & FLAG_BLKSORT else n


class ContainerError(ValueError):
    pass


class ChecksumError(ContainerError):
    """Decoded bytes whose CRC-32 differs from the container's: `index` is the first such block (RCXB) or item (RCXI),
    counted as the container counts them."""

    def __init__(self, kind: str, index: int):
        self.kind, self.index = kind, int(index)
        super().__init__(f"checksum mismatch in {kind} {self.index}")


def _version_and_flags(flags: int, crcs, count: int):
    """A header's version byte, flags and CRC table: version 1 as it always was, version 2 = the CRC bit + the table."""
    if crcs is None:
        if flags & FLAG_CRC32:
            raise ContainerError("the checksum flag needs the checksums")
        return VERSION, flags, b""
    crcs = np.ascontiguousarray(crcs, dtype="<u4")
    if len(crcs) != count:
        raise ContainerError("one checksum per block or item")
    return VERSION_CRC, flags | FLAG_CRC32, crcs.tobytes()


def _check_version(version: int, flags: int, known: int) -> bool:
    """-> whether a CRC table follows.  Version 1: exactly the flags it always had; version 2: only with the CRC bit."""
    if version == VERSION and not flags & ~known:
        return False
    if version == VERSION_CRC and flags & FLAG_CRC32 and not flags & ~(known | FLAG_CRC32):
        return True
    raise ContainerError("unsupported container version, coder or flags")


def _block_lengths(m: int, block: int, nblocks: int) -> np.ndarray:
    lengths = np.full(nblocks, block, dtype=np.int64)
    if nblocks:
        lengths[-1] = m - (nblocks - 1) * block
    return lengths


def _stored_must_fit(stored, offsets, m: int, block: int) -> None:
    """A stored block's stream is the block: its two offsets are len_b apart."""
    sizes = np.diff(np.asarray(offsets).astype(np.int64))
    if np.any(sizes[stored] != _block_lengths(m, block, len(sizes))[stored]):
        raise ContainerError("a stored block is not as long as its bytes")


def _bitmap_bytes(stored, offsets, m: int, block: int) -> bytes:
    """The bitmap of a version 3 header, b"" if no block is stored (then the header is the one without the option)."""
    if stored is None:
        return b""
    stored = np.asarray(stored) != 0
    if len(stored) != len(offsets) - 1:
        raise ContainerError("one stored flag per block")
    if not stored.any():
        return b""
    _stored_must_fit(stored, offsets, m, block)
    return np.packbits(stored, bitorder="little").tobytes()


def _parse_bitmap(buf, end: int, nblocks: int):
    """-> (stored bool[nblocks], where the bitmap ends)"""
    size = (nblocks + 7) // 8
    if nblocks > len(buf) or len(buf) < end + size:
        raise ContainerError("truncated bitmap")
    bits = np.unpackbits(np.frombuffer(bytes(buf[end: end + size]), dtype=np.uint8), bitorder="little")
    if bits[nblocks:].any():
        raise ContainerError("a padding bit of the bitmap is set")
    if not bits[:nblocks].any():
        raise ContainerError("version 3 without a stored block")
    return bits[:nblocks].astype(bool), end + size


def header_bytes(coder: int, block: int, n: int, offsets, flags: int = 0, crcs=None, stored=None) -> bytes:
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    nblocks = len(offsets) - 1
    if flags & FLAG_STORED:
        raise ContainerError("the stored flag comes with the bitmap")
    if nblocks != (coded_size(n, flags) + block - 1) // block:
        raise ContainerError("offsets do not match n and the block size")
    bitmap = _bitmap_bytes(stored, offsets, coded_size(n, flags), block)
    version, flags, table = _version_and_flags(flags, crcs, nblocks)
    if bitmap:
        version, flags = VERSION_STORED, flags | FLAG_STORED
    return _FIXED.pack(MAGIC, version, coder, flags, block, n, nblocks) + offsets.tobytes() + bitmap + table


def parse(blob):
    """-> dict(coder, flags, block, n, nblocks, offsets uint64[nblocks+1], crcs uint32[nblocks] or None, stored bool[nblocks] or None,
    payload uint8 view)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, block, n, nblocks = _FIXED.unpack(bytes(buf[: _FIXED.size]))
    if magic != MAGIC:
        raise ContainerError("not an RCXB container")
    if coder not in (0, 1, 2, 3):
        raise ContainerError("unsupported container version, coder or flags")
    if version == VERSION_STORED:  # always with its flag; bits 0 and 1 as in the versions before
        if not flags & FLAG_STORED or flags & ~(FLAG_BLKSORT | FLAG_CRC32 | FLAG_STORED):
            raise ContainerError("unsupported container version, coder or flags")
        checked = bool(flags & FLAG_CRC32)
    else:
        checked = _check_version(version, flags, FLAG_BLKSORT)
    if block < 16 or block > (1 << 24) - 256 or nblocks != (coded_size(n, flags) + block - 1) // block:
        raise ContainerError("inconsistent header")
    end = _FIXED.size + 8 * (nblocks + 1)
    if len(buf) < end:
        raise ContainerError("truncated offset table")
    offsets = np.frombuffer(bytes(buf[_FIXED.size:end]), dtype="<u8").astype(np.uint64)
    stored = None
    if version == VERSION_STORED:
        stored, end = _parse_bitmap(buf, end, nblocks)
    crcs = None
    if checked:
        if nblocks > len(buf) or len(buf) < end + 4 * nblocks:
            raise ContainerError("truncated checksum table")
        crcs = np.frombuffer(bytes(buf[end: end + 4 * nblocks]), dtype="<u4").astype(np.uint32)
        end += 4 * nblocks
    if offsets[0] != 0 or np.any(np.diff(offsets.astype(np.int64)) < 0) or end + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    if stored is not None:
        _stored_must_fit(stored, offsets, coded_size(n, flags), block)
    return {"coder": coder, "flags": flags, "block": block, "n": n, "nblocks": nblocks, "offsets": offsets, "crcs": crcs, "stored": stored,
            "payload": buf[end:]}


# ---- the checked paths: one upload, the device calls, one download ------------------------------------------------
def _cuda(a, dtype=None):
    import torch
    a = np.array(a, dtype=dtype)  # (a writable copy: a container's arrays are views of the caller's bytes)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _crcs_of(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).copy()


def _gain(stored):
    """The option stored=None | True | fraction of pack and pack_typed -> None, or the gain of include/rcx_stored.h."""
    if stored is None or stored is False:
        return None
    from . import stored as calls
    try:
        return calls.gain_q16(stored)
    except ValueError as e:
        raise ContainerError(f"stored is None, True or a fraction 0 <= g < 1 of the block, not {stored!r}") from e


def _mix_device(ctx, d_src, block: int, d_dst, d_offs, gain: int):
    """Behind the encode call on d_src: the mix of include/rcx_stored.h -> (mixed streams, their table, the flags), on the device."""
    import torch
    from . import rcx, stored as calls
    nblocks = rcx.block_count(d_src.numel(), block)
    d_mixed = torch.empty(d_src.numel(), dtype=torch.uint8, device="cuda")  # a mixed payload is never longer than the text
    d_moffs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(nblocks, dtype=torch.uint8, device="cuda")
    calls.mix_device(ctx, d_src, block, d_dst, d_dst.numel(), d_offs, gain, d_mixed, d_moffs, d_flags)
    return d_mixed, d_moffs, d_flags


def _pack_device(ctx, src: np.ndarray, block: int, coder: int, blksort: bool, checksum: bool = True, gain=None):
    """-> (payload, offsets, crcs or None, stored flags or None): block sort (if asked for), encode, the mix of the stored blocks
    (if asked for) and CRC-32 of the coder's input (if asked for), all on the device."""
    import torch
    from . import rcx
    d_src = _cuda(src)
    if blksort:
        d_sorted = torch.empty(rcx.bwt_encode_bound(len(src)), dtype=torch.uint8, device="cuda")
        ctx.bwt_encode_device(d_src, d_sorted)
        d_src = d_sorted[: coded_size(len(src), FLAG_BLKSORT)]
    m = d_src.numel()
    nblocks = rcx.block_count(m, block)
    d_dst = torch.empty(rcx.encode_bound(m, block, coder), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
    d_crc = torch.zeros(nblocks, dtype=torch.int32, device="cuda")
    ctx.encode_blocks_device(d_src, block, d_dst, d_offs, coder=coder)
    d_flags = None
    if gain is not None:
        d_dst, d_offs, d_flags = _mix_device(ctx, d_src, block, d_dst, d_offs, gain)
    if checksum:
        ctx.crc32_blocks_device(d_src, block, d_crc)
    ctx.sync_status()
    offsets = d_offs.cpu().numpy().astype(np.uint64)
    return (d_dst[: int(offsets[-1])].cpu().numpy(), offsets, _crcs_of(d_crc) if checksum else None,
            None if d_flags is None else d_flags.cpu().numpy())


def _sync_checked(ctx, kind: str, name=lambda k: k):
    """The latch behind a verify call: a mismatch becomes ChecksumError with the container's index."""
    from . import rcx
    st, bad = ctx.sync_status(raise_on_error=False)
    if st == rcx.E_CORRUPT:
        raise ChecksumError(kind, name(int(bad)))
    if st != rcx.OK:
        raise rcx.RcxError(st, f"{kind} {bad}")


def _decode_all_device(ctx, c, m: int, d_out) -> None:
    """Every block of a container to d_out: through the block call, or with stored blocks through the call that copies them."""
    if c.get("stored") is None:
        ctx.decode_blocks_device(_cuda(c["payload"]), len(c["payload"]), _cuda(c["offsets"]), m, c["block"], d_out, coder=c["coder"])
    else:
        from . import stored as calls
        doffs = np.minimum(np.arange(c["nblocks"] + 1, dtype=np.uint64) * np.uint64(c["block"]), np.uint64(m))
        calls.decode_device(ctx, _cuda(c["payload"]), len(c["payload"]), _cuda(c["offsets"]), c["stored"], doffs, d_out, coder=c["coder"])
    ctx.sync_status()  # (the decoder's own failures first: a stream that runs dry is an RcxError, as without checksums)


def _unpack_device(ctx, c, verify: bool = True) -> bytes:
    import torch
    m = coded_size(c["n"], c["flags"])
    d_out = torch.empty(m, dtype=torch.uint8, device="cuda")
    _decode_all_device(ctx, c, m, d_out)
    if verify and c["crcs"] is not None:
        ctx.verify_blocks_device(d_out, c["block"], _cuda(c["crcs"]))
        _sync_checked(ctx, "block")
    if c["flags"] & FLAG_BLKSORT:
        d_text = torch.empty(max(c["n"], 1), dtype=torch.uint8, device="cuda")
        ctx.bwt_decode_device(d_out, m, d_text)
        ctx.sync_status()
        d_out = d_text[: c["n"]]
    return d_out.cpu().numpy().tobytes()


def _decode_picked_device(ctx, c, lengths, pick, kind: str, checked: bool):
    """Streams pick[k] of a container, decoded back to back on the device and, if `checked`, verified there
    -> (the device buffer, the table of where each pick lies in it)."""
    import torch
    from . import rcx
    pick = np.asarray(pick, dtype=np.uint64)
    doffs = rcx.item_offsets(np.asarray(lengths, dtype=np.uint64)[pick.astype(np.int64)])
    d_out = torch.empty(max(int(doffs[-1]), 1), dtype=torch.uint8, device="cuda")
    if c.get("stored") is None:
        ctx.decode_items_device(_cuda(c["payload"]), len(c["payload"]), _cuda(c["offsets"]), doffs, d_out, pick=pick, coder=c["coder"])
    else:
        from . import stored as calls
        calls.decode_device(ctx, _cuda(c["payload"]), len(c["payload"]), _cuda(c["offsets"]), c["stored"], doffs, d_out, pick=pick, coder=c["coder"])
    ctx.sync_status()
    if checked:
        ctx.verify_items_device(d_out, doffs, _cuda(c["crcs"][pick.astype(np.int64)]))
        _sync_checked(ctx, kind, lambda k: int(pick[k]))
    return d_out, doffs


def _decode_picked_checked(ctx, c, lengths, pick, kind: str) -> list:
    """Streams pick[k] of a checked container, decoded back to back and verified -> their bytes."""
    d_out, doffs = _decode_picked_device(ctx, c, lengths, pick, kind, True)
    out = d_out.cpu().numpy()
    return [out[int(doffs[k]): int(doffs[k + 1])] for k in range(len(pick))]


def pack(data, block: int = 65536, coder: int = 0, ctx=None, blksort: bool = False, checksum: bool = False, stored=None) -> bytes:
    """stored=True | fraction: blocks that do not shrink (by that fraction of their length) are kept raw, see the module's
    docstring; the container is version 3 if there is such a block, else the one written without the option."""
    from . import rcx
    gain = _gain(stored)
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        src = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        flags = FLAG_BLKSORT if blksort else 0
        if len(src) == 0:
            return header_bytes(coder, block, 0, np.zeros(1, np.uint64), flags, np.zeros(0, np.uint32) if checksum else None)
        if checksum or gain is not None:
            payload, offsets, crcs, raw = _pack_device(ctx, src, block, coder, blksort, checksum, gain)
            return header_bytes(coder, block, len(src), offsets, flags, crcs, raw) + payload.tobytes()
        payload, offsets = ctx.encode_blocks(ctx.bwt_encode(src) if blksort else src, block, coder=coder)
        return header_bytes(coder, block, len(src), offsets, flags) + payload.tobytes()
    finally:
        if own:
            ctx.close()


def unpack(blob, ctx=None, verify: bool = True) -> bytes:
    from . import rcx
    c = parse(blob)
    if c["n"] == 0:
        return b""
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        if (verify and c["crcs"] is not None) or c["stored"] is not None:
            return _unpack_device(ctx, c, verify)
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


def unpack_range(blob, start: int, stop: int, ctx=None, verify: bool = True) -> bytes:
    """The bytes [start, stop) of the original, decoding -- and, in a container with checksums, verifying -- only the
    blocks that cover them."""
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
        if verify and c["crcs"] is not None:
            parts = _decode_picked_checked(ctx, c, lengths, pick, "block")
        elif c["stored"] is not None:
            d_out, doffs = _decode_picked_device(ctx, c, lengths, pick, "block", False)
            parts = [d_out[: int(doffs[-1])].cpu().numpy()]
        else:
            parts = ctx.decode_items(c["payload"], c["offsets"], lengths, pick=pick, coder=c["coder"])
    finally:
        if own:
            ctx.close()
    out = np.concatenate(parts)
    return out[start - first * block: stop - first * block].tobytes()


def item_header_bytes(coder: int, lengths, offsets, crcs=None) -> bytes:
    lengths = np.ascontiguousarray(lengths, dtype="<u8")
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    if len(offsets) != len(lengths) + 1:
        raise ContainerError("offsets do not match the number of items")
    if len(lengths) and int(lengths.max()) > MAX_ITEM:
        raise ContainerError("an item is longer than the coder takes")
    version, flags, table = _version_and_flags(0, crcs, len(lengths))
    return _ITEM_FIXED.pack(ITEM_MAGIC, version, coder, flags, len(lengths)) + lengths.tobytes() + offsets.tobytes() + table


def parse_items(blob):
    """-> dict(coder, nitems, lengths uint64[nitems], offsets uint64[nitems+1], crcs uint32[nitems] or None, payload uint8 view)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _ITEM_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, nitems = _ITEM_FIXED.unpack(bytes(buf[: _ITEM_FIXED.size]))
    if magic != ITEM_MAGIC:
        raise ContainerError("not an RCXI container")
    if coder not in (0, 1, 2, 3):
        raise ContainerError("unsupported container version, coder or flags")
    checked = _check_version(version, flags, 0)
    mid = _ITEM_FIXED.size + 8 * nitems
    end = mid + 8 * (nitems + 1)
    if nitems > len(buf) or len(buf) < end:
        raise ContainerError("truncated tables")
    lengths = np.frombuffer(bytes(buf[_ITEM_FIXED.size:mid]), dtype="<u8").astype(np.uint64)
    offsets = np.frombuffer(bytes(buf[mid:end]), dtype="<u8").astype(np.uint64)
    crcs = None
    if checked:
        if len(buf) < end + 4 * nitems:
            raise ContainerError("truncated checksum table")
        crcs = np.frombuffer(bytes(buf[end: end + 4 * nitems]), dtype="<u4").astype(np.uint32)
        end += 4 * nitems
    if nitems and int(lengths.max()) > MAX_ITEM:
        raise ContainerError("an item is longer than the coder takes")
    sizes = np.diff(offsets.astype(np.int64))
    if offsets[0] != 0 or np.any(sizes < 0) or end + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    if np.any((lengths == 0) != (sizes == 0)):
        raise ContainerError("an item of length 0 has no stream, and only such an item")
    return {"coder": coder, "nitems": nitems, "lengths": lengths, "offsets": offsets, "crcs": crcs, "payload": buf[end:]}


def pack_items(items, coder: int = 0, ctx=None, checksum: bool = False) -> bytes:
    """items: a list of buffers -> an RCXI container."""
    from . import rcx
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        parts = [np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if not isinstance(x, np.ndarray) else x, dtype=np.uint8) for x in items]
        if checksum:
            import torch
            soffs = rcx.item_offsets([len(x) for x in parts])
            d_src = _cuda(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
            d_dst = torch.empty(max(rcx.encode_items_bound(soffs, coder), 1), dtype=torch.uint8, device="cuda")
            d_offs = torch.zeros(len(soffs), dtype=torch.int64, device="cuda")
            d_crc = torch.zeros(len(parts), dtype=torch.int32, device="cuda")
            ctx.encode_items_device(d_src, soffs, d_dst, d_offs, coder=coder)
            ctx.crc32_items_device(d_src, soffs, d_crc)
            ctx.sync_status()
            offsets = d_offs.cpu().numpy().astype(np.uint64)
            return item_header_bytes(coder, [len(x) for x in parts], offsets, _crcs_of(d_crc)) + d_dst[: int(offsets[-1])].cpu().numpy().tobytes()
        payload, offsets = ctx.encode_items(parts, coder=coder)
        return item_header_bytes(coder, [len(x) for x in parts], offsets) + payload.tobytes()
    finally:
        if own:
            ctx.close()


def unpack_items(blob, pick=None, ctx=None, verify: bool = True) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None); picks may repeat.  In a container
    with checksums the picked items, and only they, are verified."""
    from . import rcx
    c = parse_items(blob)
    if pick is not None and any(not 0 <= int(k) < c["nitems"] for k in pick):
        raise ContainerError("no such item")
    if c["nitems"] == 0 or (pick is not None and len(pick) == 0):
        return []
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        if verify and c["crcs"] is not None:
            picked = np.arange(c["nitems"], dtype=np.uint64) if pick is None else pick
            return [x.tobytes() for x in _decode_picked_checked(ctx, c, c["lengths"], picked, "item")]
        return [x.tobytes() for x in ctx.decode_items(c["payload"], c["offsets"], c["lengths"], pick=pick, coder=c["coder"])]
    finally:
        if own:
            ctx.close()


# ---- the typed container: the byte-plane filter in front of the coder ---------------------------------------------------
def typed_header_bytes(coder: int, block: int, n: int, width: int, offsets, crcs=None, pred: int = 0, stored=None) -> bytes:
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    nblocks = len(offsets) - 1
    if width not in WIDTHS:
        raise ContainerError("an element is 2, 4 or 8 bytes wide")
    if type(pred) is not int or pred not in (0, 1, 2):
        raise ContainerError("a predictor is 0 (none), 1 (delta) or 2 (zigzag)")
    if nblocks != (n + block - 1) // block:
        raise ContainerError("offsets do not match n and the block size")
    flags, table = 0, b""
    if crcs is not None:
        crcs = np.ascontiguousarray(crcs, dtype="<u4")
        if len(crcs) != nblocks:
            raise ContainerError("one checksum per block or item")
        flags, table = FLAG_CRC32, crcs.tobytes()
    version = TYPED_VERSION_PRED if pred else TYPED_VERSION  # version 2 only with a predictor
    bitmap = _bitmap_bytes(stored, offsets, n, block)
    if bitmap:  # version 3 only with a stored block
        version, flags = TYPED_VERSION_STORED, flags | FLAG_STORED
    return (_TYPED_FIXED.pack(TYPED_MAGIC, version, coder, flags, block, n, nblocks, width, bytes([pred]) + bytes(6)) + offsets.tobytes() + bitmap
            + table)


def parse_typed(blob):
    """-> dict(coder, flags, block, n, nblocks, width, pred, offsets uint64[nblocks+1], crcs uint32[nblocks] or None, stored bool[nblocks]
    or None, payload uint8 view); pred is 0 for a version 1 container"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _TYPED_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, block, n, nblocks, width, reserved = _TYPED_FIXED.unpack(bytes(buf[: _TYPED_FIXED.size]))
    if magic != TYPED_MAGIC:
        raise ContainerError("not an RCXT container")
    known = FLAG_CRC32 | (FLAG_STORED if version == TYPED_VERSION_STORED else 0)  # bit 2 in version 3, and always there
    if (version not in (TYPED_VERSION, TYPED_VERSION_PRED, TYPED_VERSION_STORED) or coder not in (0, 1, 2, 3) or flags & ~known
            or (version == TYPED_VERSION_STORED and not flags & FLAG_STORED)):
        raise ContainerError("unsupported container version, coder or flags")
    pred = reserved[0]
    pred_ok = pred in (1, 2) if version == TYPED_VERSION_PRED else pred in (0, 1, 2) if version == TYPED_VERSION_STORED else pred == 0
    if width not in WIDTHS or reserved[1:] != bytes(6) or not pred_ok:
        raise ContainerError("an element is 2, 4 or 8 bytes wide, version 2 names its predictor, and the reserved bytes are zero")
    if block < 16 or block > (1 << 24) - 256 or nblocks != (n + block - 1) // block:
        raise ContainerError("inconsistent header")
    end = _TYPED_FIXED.size + 8 * (nblocks + 1)
    if nblocks > len(buf) or len(buf) < end:
        raise ContainerError("truncated offset table")
    offsets = np.frombuffer(bytes(buf[_TYPED_FIXED.size:end]), dtype="<u8").astype(np.uint64)
    stored = None
    if version == TYPED_VERSION_STORED:
        stored, end = _parse_bitmap(buf, end, nblocks)
    crcs = None
    if flags & FLAG_CRC32:
        if len(buf) < end + 4 * nblocks:
            raise ContainerError("truncated checksum table")
        crcs = np.frombuffer(bytes(buf[end: end + 4 * nblocks]), dtype="<u4").astype(np.uint32)
        end += 4 * nblocks
    if offsets[0] != 0 or np.any(np.diff(offsets.astype(np.int64)) < 0) or end + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    if stored is not None:
        _stored_must_fit(stored, offsets, n, block)
    return {"coder": coder, "flags": flags, "block": block, "n": n, "nblocks": nblocks, "width": width, "pred": pred, "offsets": offsets,
            "crcs": crcs, "stored": stored, "payload": buf[end:]}


def _typed_source(data, width):
    """-> (the bytes: a uint8 cuda tensor if `data` lies on the GPU, else a uint8 numpy array; the element width)"""
    if type(data).__module__.split(".")[0] == "torch":
        import torch
        if not data.is_contiguous():
            raise ContainerError("a tensor must be contiguous")
        width = data.element_size() if width is None else width
        flat = data.detach().reshape(-1).view(torch.uint8)
        src = flat if flat.is_cuda else flat.numpy()
    elif isinstance(data, np.ndarray):
        width = data.dtype.itemsize if width is None else width
        src = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        src = np.frombuffer(data, dtype=np.uint8)
    if width is None:
        raise ContainerError("plain bytes have no element size: give the width")
    if width not in WIDTHS:
        raise ContainerError(f"an element is 2, 4 or 8 bytes wide, not {width}")
    return src, width


def pick_predictor(c_none: int, c_delta: int, c_zigzag: int):
    """The rule of predict="auto" on the three costs (any one unit) -> None, "delta" or "zigzag": the cheaper of the
    predictors that earn at least 1/64 of the cost without one, delta on a tie; None if neither does."""
    best = None
    for name, c in (("delta", int(c_delta)), ("zigzag", int(c_zigzag))):
        if 64 * c < 63 * int(c_none) and (best is None or c < best[1]):
            best = (name, c)
    return best[0] if best else None


def _measured_predictor(ctx, d_src, width: int, block: int, nblocks: int, d_split):
    """-> (the rule's pick, the predictor whose split text d_split holds now).  Three splits into d_split, a statistics pass
    over each (costs only), three sums in one download."""
    import torch
    from . import predict as predictor, stats
    d_cost = torch.empty(3 * nblocks, dtype=torch.int64, device="cuda")
    for pred in (0, 1, 2):
        predictor.split_device(ctx, d_src, width, block, pred, d_split)
        stats.blocks_device(ctx, d_split, block, None, d_cost[pred * nblocks: (pred + 1) * nblocks])
    totals = [int(v) for v in d_cost.view(3, nblocks).sum(dim=1).cpu()]  # (a block's cost is below 2^45)
    return pick_predictor(*totals), 2


def pack_typed(data, width=None, block: int = 65536, coder: int = 0, ctx=None, checksum: bool = False, predict=None, stored=None) -> bytes:
    """data: bytes, a numpy array or a contiguous torch tensor (CPU or GPU) -> an RCXT container.  width=None: the
    element size of the array or tensor.  predict=None, "delta" or "zigzag": the predictor of include/rcx_predict.h in front of
    the filter, for integers whose differences are small (unsorted data gets worse by it).  predict="auto": the one the
    rule in this module's docstring picks from the measured order-0 costs, or none; the container is the one that choice
    given by name writes.  That costs up to four splits and three statistics passes where a named choice costs one split:
    measured on a GiB of sorted int64 keys at 64 KiB blocks, 2.33 ms for the decision beside 4.86 ms for the adaptive
    encode that follows, 48 % of it (profiles/r08_stats_rate.jsonl).  One upload (none for a GPU
    tensor), then split, encode and, with checksum=True, the CRC-32 of every block of the split text, all with the device
    calls.  stored=True | fraction: blocks of the split text that do not shrink (by that fraction) are kept raw -- the low
    mantissa planes of floating-point data -- and the container is version 3 if there is one (the module's docstring)."""
    gain = _gain(stored)
    auto = isinstance(predict, str) and predict == AUTO
    if not auto and (not (predict is None or isinstance(predict, str)) or predict not in PREDICTORS):
        raise ContainerError(f"a predictor is None, 'delta', 'zigzag' or 'auto', not {predict!r}")
    pred = 0 if auto else PREDICTORS[predict]  # (nothing to measure in an empty buffer: none, version 1)
    src, width = _typed_source(data, width)
    import torch
    from . import predict as predictor, rcx
    n = int(src.numel()) if hasattr(src, "numel") else len(src)
    if n == 0:
        return typed_header_bytes(coder, block, 0, width, np.zeros(1, np.uint64), np.zeros(0, np.uint32) if checksum else None, pred)
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        d_src = src if hasattr(src, "numel") else _cuda(src)
        nblocks = rcx.block_count(n, block)
        d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_dst = torch.empty(rcx.encode_bound(n, block, coder), dtype=torch.uint8, device="cuda")
        d_offs = torch.zeros(nblocks + 1, dtype=torch.int64, device="cuda")
        held = None  # the predictor whose split text d_split holds
        if auto:
            choice, held = _measured_predictor(ctx, d_src, width, block, nblocks, d_split)
            pred = PREDICTORS[choice]
        if held != pred:
            predictor.split_device(ctx, d_src, width, block, pred, d_split)  # (no predictor: the plane filter's own kernel)
        ctx.encode_blocks_device(d_split, block, d_dst, d_offs, coder=coder)
        d_flags = None
        if gain is not None:
            d_dst, d_offs, d_flags = _mix_device(ctx, d_split, block, d_dst, d_offs, gain)
        crcs = None
        if checksum:
            d_crc = torch.zeros(nblocks, dtype=torch.int32, device="cuda")
            ctx.crc32_blocks_device(d_split, block, d_crc)
        ctx.sync_status()
        if checksum:
            crcs = _crcs_of(d_crc)
        offsets = d_offs.cpu().numpy().astype(np.uint64)
        raw = None if d_flags is None else d_flags.cpu().numpy()
        return typed_header_bytes(coder, block, n, width, offsets, crcs, pred, raw) + d_dst[: int(offsets[-1])].cpu().numpy().tobytes()
    finally:
        if own:
            ctx.close()


def unpack_typed(blob, ctx=None, verify: bool = True) -> bytes:
    """Decode, verify the split text block by block if the container carries checksums (verify=False skips that), join."""
    import torch
    from . import predict as predictor, rcx
    c = parse_typed(blob)
    n = c["n"]
    if n == 0:
        return b""
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
        _decode_all_device(ctx, c, n, d_split)
        if verify and c["crcs"] is not None:
            ctx.verify_blocks_device(d_split, c["block"], _cuda(c["crcs"]))
            _sync_checked(ctx, "block")
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        predictor.join_device(ctx, d_split, c["width"], c["block"], c["pred"], d_out)
        return d_out.cpu().numpy().tobytes()
    finally:
        if own:
            ctx.close()


def unpack_typed_range(blob, start: int, stop: int, ctx=None, verify: bool = True) -> bytes:
    """The bytes [start, stop) of the original: only the blocks of the superblocks that cover them are decoded and, in a
    container with checksums, verified; their span is joined as a buffer of its own."""
    import torch
    from . import predict as predictor, rcx
    c = parse_typed(blob)
    n, block, width, nblocks = c["n"], c["block"], c["width"], c["nblocks"]
    if not 0 <= start <= stop <= n:
        raise ContainerError("range outside the data")
    if start == stop:
        return b""
    superblock = width * block
    first, last = start // superblock, (stop - 1) // superblock
    pick = np.arange(first * width, min(nblocks, (last + 1) * width), dtype=np.uint64)
    lengths = np.full(nblocks, block, dtype=np.uint64)
    lengths[-1] = n - (nblocks - 1) * block
    span = min(n, (last + 1) * superblock) - first * superblock
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        # the picked blocks follow one another and all but the container's last are whole: back to back they are the span's split text
        d_split, doffs = _decode_picked_device(ctx, c, lengths, pick, "block", verify and c["crcs"] is not None)
        if int(doffs[-1]) != span:
            raise ContainerError("decoded size differs from the header")
        d_out = torch.empty(span, dtype=torch.uint8, device="cuda")
        predictor.join_device(ctx, d_split[:span], width, block, c["pred"], d_out)
        out = d_out.cpu().numpy()
    finally:
        if own:
            ctx.close()
    return out[start - first * superblock: stop - first * superblock].tobytes()


# ---- the typed item container: a width and a predictor per buffer, in front of the item calls ---------------------------
TYPED_ITEMS_MAGIC = b"RCXJ"
TYPED_ITEMS_VERSION = 1
_TYPED_ITEMS_FIXED = struct.Struct("<4sBBHQQQ")
ITEM_WIDTHS = (1, 2, 4, 8)


def _sub_lengths(lengths, widths) -> np.ndarray:
    """The sub-items' lengths (int64): item i gives widths[i] of len // width bytes, the last with the len % width tail."""
    lengths, widths = np.asarray(lengths).astype(np.int64), np.asarray(widths).astype(np.int64)
    m = lengths // np.maximum(widths, 1)
    sub = np.repeat(m, widths)
    if len(widths):
        sub[np.cumsum(widths) - 1] += lengths - m * widths
    return sub


def _typed_items_tables(lengths, widths, preds):
    lengths = np.ascontiguousarray(lengths, dtype="<u8")
    widths = np.ascontiguousarray(widths, dtype=np.uint8)
    preds = np.zeros(len(widths), np.uint8) if preds is None else np.ascontiguousarray(preds, dtype=np.uint8)
    if len(widths) != len(lengths) or len(preds) != len(lengths):
        raise ContainerError("one length, one width and one predictor per item")
    if np.any(~np.isin(widths, ITEM_WIDTHS)):
        raise ContainerError("an element is 1, 2, 4 or 8 bytes wide")
    if np.any(preds > 2) or np.any((widths == 1) & (preds != 0)):
        raise ContainerError("a predictor is 0 (none), 1 (delta) or 2 (zigzag), and 0 for width 1")
    sub = _sub_lengths(lengths, widths)
    if len(sub) and int(sub.max()) > MAX_ITEM:
        raise ContainerError("a sub-item is longer than the coder takes")
    return lengths, widths, preds, sub


def typed_items_header_bytes(coder: int, lengths, widths, preds, offsets, crcs=None, directory: bytes = b"") -> bytes:
    lengths, widths, preds, sub = _typed_items_tables(lengths, widths, preds)
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    if len(offsets) != len(sub) + 1:
        raise ContainerError("offsets do not match the number of sub-items")
    flags, table = 0, b""
    if crcs is not None:
        crcs = np.ascontiguousarray(crcs, dtype="<u4")
        if len(crcs) != len(sub):
            raise ContainerError("one checksum per sub-item")
        flags, table = FLAG_CRC32, crcs.tobytes()
    directory = bytes(directory)
    return (_TYPED_ITEMS_FIXED.pack(TYPED_ITEMS_MAGIC, TYPED_ITEMS_VERSION, coder, flags, len(lengths), len(sub), len(directory)) + lengths.tobytes()
            + widths.tobytes() + preds.tobytes() + offsets.tobytes() + table + directory)


def parse_typed_items(blob):
    """-> dict(coder, flags, nitems, nsub, lengths uint64[nitems], widths uint8[nitems], preds uint8[nitems], sub_first int64[nitems + 1],
    sub_lengths uint64[nsub], offsets uint64[nsub + 1], crcs uint32[nsub] or None, directory bytes, payload uint8 view)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _TYPED_ITEMS_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, coder, flags, nitems, nsub, dlen = _TYPED_ITEMS_FIXED.unpack(bytes(buf[: _TYPED_ITEMS_FIXED.size]))
    if magic != TYPED_ITEMS_MAGIC:
        raise ContainerError("not an RCXJ container")
    if version != TYPED_ITEMS_VERSION or coder not in (0, 1, 2, 3) or flags & ~FLAG_CRC32:
        raise ContainerError("unsupported container version, coder or flags")
    at = _TYPED_ITEMS_FIXED.size
    if nitems > len(buf) or nsub > len(buf) or dlen > len(buf) or len(buf) < at + 10 * nitems + 8 * (nsub + 1):
        raise ContainerError("truncated tables")
    lengths = np.frombuffer(bytes(buf[at: at + 8 * nitems]), dtype="<u8").astype(np.uint64)
    at += 8 * nitems
    widths = np.array(buf[at: at + nitems], dtype=np.uint8)
    preds = np.array(buf[at + nitems: at + 2 * nitems], dtype=np.uint8)
    at += 2 * nitems
    _, _, _, sub = _typed_items_tables(lengths, widths, preds)  # (refuses bad widths and predictors, and sub-items that are too long)
    if len(sub) != nsub:
        raise ContainerError("the widths do not add up to the number of sub-items")
    offsets = np.frombuffer(bytes(buf[at: at + 8 * (nsub + 1)]), dtype="<u8").astype(np.uint64)
    at += 8 * (nsub + 1)
    crcs = None
    if flags & FLAG_CRC32:
        if len(buf) < at + 4 * nsub:
            raise ContainerError("truncated checksum table")
        crcs = np.frombuffer(bytes(buf[at: at + 4 * nsub]), dtype="<u4").astype(np.uint32)
        at += 4 * nsub
    if len(buf) < at + dlen:
        raise ContainerError("truncated directory")
    directory = bytes(buf[at: at + dlen])
    at += dlen
    sizes = np.diff(offsets.astype(np.int64))
    if offsets[0] != 0 or np.any(sizes < 0) or at + int(offsets[-1]) != len(buf):
        raise ContainerError("offset table does not match the payload")
    if np.any((sub == 0) != (sizes == 0)):
        raise ContainerError("a sub-item of length 0 has no stream, and only such a sub-item")
    sub_first = np.concatenate([[0], np.cumsum(widths.astype(np.int64))])
    return {"coder": coder, "flags": flags, "nitems": nitems, "nsub": nsub, "lengths": lengths, "widths": widths, "preds": preds, "sub_first": sub_first,
            "sub_lengths": sub.astype(np.uint64), "offsets": offsets, "crcs": crcs, "directory": directory, "payload": buf[at:]}


def _item_source(x):
    """One item -> (its bytes: a uint8 cuda tensor if it lies on the GPU, else a uint8 numpy array; its element size or None)"""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        if not x.is_contiguous():
            raise ContainerError("a tensor must be contiguous")
        flat = x.detach().reshape(-1).view(torch.uint8)
        return (flat if flat.is_cuda else flat.numpy()), x.element_size()
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).reshape(-1).view(np.uint8), x.dtype.itemsize
    return np.frombuffer(x, dtype=np.uint8), None


def _gather_device(parts):
    """The items' bytes back to back on the device: no upload if all of them lie there, else one."""
    import torch
    if not parts:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    if all(hasattr(x, "is_cuda") for x in parts):
        return torch.cat(parts) if len(parts) > 1 else parts[0]
    return _cuda(np.concatenate([x.cpu().numpy() if hasattr(x, "is_cuda") else x for x in parts]))


def _item_predictors(predict, widths):
    """predict: None, a name, AUTO or one entry per item -> (preds uint8[nitems] with 0 where it is measured, auto bool[nitems])"""
    nitems = len(widths)
    entries = list(predict) if isinstance(predict, (list, tuple)) else [predict] * nitems
    if len(entries) != nitems:
        raise ContainerError("one predictor per item")
    preds, auto = np.zeros(nitems, np.uint8), np.zeros(nitems, bool)
    for i, e in enumerate(entries):
        if isinstance(e, str) and e == AUTO:
            auto[i] = widths[i] > 1  # (a width-1 item is never predicted)
        elif (e is None or isinstance(e, str)) and e in PREDICTORS:
            if e is not None and widths[i] == 1:
                if isinstance(predict, (list, tuple)):
                    raise ContainerError("an item of width 1 takes no predictor")
            else:
                preds[i] = PREDICTORS[e]
        else:
            raise ContainerError(f"a predictor is None, 'delta', 'zigzag' or 'auto', not {e!r}")
    return preds, auto


def _measured_item_predictors(ctx, d_src, offs, widths, sub_offs, preds, auto, d_split):
    """The items marked in `auto` get pick_predictor's choice on the sums of their sub-items' order-0 costs under none, delta and
    zigzag: three segmented splits into d_split, a statistics pass over each (costs only), one download of the sums."""
    import torch
    from . import stats, typed_items
    nsub, nitems = len(sub_offs) - 1, len(widths)
    d_cost = torch.zeros(3 * nsub, dtype=torch.int64, device="cuda")
    for cand in (0, 1, 2):
        typed_items.split_device(ctx, d_src, offs, widths, np.where(auto, cand, preds).astype(np.uint8), d_split)
        stats.items_device(ctx, d_split, sub_offs, None, d_cost[cand * nsub: (cand + 1) * nsub])
    # the sums per item: differences of the running sum at the items' sub-item borders (a sub-item's cost is below 2^45)
    running = torch.cat([torch.zeros(3, 1, dtype=torch.int64, device="cuda"), torch.cumsum(d_cost.view(3, nsub), dim=1)], dim=1)
    borders = torch.from_numpy(np.concatenate([[0], np.cumsum(widths.astype(np.int64))])).cuda()
    sums = (running[:, borders[1:]] - running[:, borders[:-1]]).cpu().numpy()
    out = preds.copy()
    for i in np.flatnonzero(auto):
        out[i] = PREDICTORS[pick_predictor(int(sums[0, i]), int(sums[1, i]), int(sums[2, i]))]
    assert sums.shape == (3, nitems)
    return out


def _pack_typed_items_device(ctx, d_src, lengths, widths, preds, auto, coder: int, checksum: bool, directory: bytes) -> bytes:
    """d_src: the items back to back on the device -> the container: split, encode over the sub-items, with checksum the CRC-32
    of the sub-items of the split text, one download."""
    import torch
    from . import rcx, typed_items
    lengths = np.asarray(lengths, dtype=np.uint64)
    _typed_items_tables(lengths, widths, preds)
    nsub = int(widths.astype(np.int64).sum())
    if int(lengths.sum()) == 0:  # nothing to code: no GPU
        return typed_items_header_bytes(coder, lengths, widths, preds, np.zeros(nsub + 1, np.uint64), np.zeros(nsub, np.uint32) if checksum else None, directory)
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        offs = rcx.item_offsets(lengths)
        sub_offs = typed_items.sub_offsets(offs, widths)
        d_split = torch.empty(d_src.numel(), dtype=torch.uint8, device="cuda")
        if auto.any():
            preds = _measured_item_predictors(ctx, d_src, offs, widths, sub_offs, preds, auto, d_split)
        typed_items.split_device(ctx, d_src, offs, widths, preds, d_split)
        d_dst = torch.empty(max(rcx.encode_items_bound(sub_offs, coder), 1), dtype=torch.uint8, device="cuda")
        d_offs = torch.zeros(nsub + 1, dtype=torch.int64, device="cuda")
        ctx.encode_items_device(d_split, sub_offs, d_dst, d_offs, coder=coder)
        crcs = None
        if checksum:
            d_crc = torch.zeros(nsub, dtype=torch.int32, device="cuda")
            ctx.crc32_items_device(d_split, sub_offs, d_crc)
        ctx.sync_status()
        if checksum:
            crcs = _crcs_of(d_crc)
        offsets = d_offs.cpu().numpy().astype(np.uint64)
        return typed_items_header_bytes(coder, lengths, widths, preds, offsets, crcs, directory) + d_dst[: int(offsets[-1])].cpu().numpy().tobytes()
    finally:
        if own:
            ctx.close()


def pack_typed_items(items, widths=None, predict=None, coder: int = 0, ctx=None, checksum: bool = False, directory: bytes = b"") -> bytes:
    """items: a list of buffers (bytes, numpy arrays, contiguous torch tensors on the CPU or the GPU) -> an RCXJ container.
    widths=None: each array's or tensor's element size (plain bytes need a width); else one width for all, or one per item.
    predict: None, "delta", "zigzag", "auto", or a list with one of these per item; "auto" decides per item from the measured
    order-0 costs (the module's docstring), and a width-1 item is never predicted.  One upload (none if every item lies on the
    GPU), then split, encode over the sub-items and, with checksum=True, their CRC-32, all with the device calls."""
    sources = [_item_source(x) for x in items]
    if widths is None:
        each = [w for _, w in sources]
        if any(w is None for w in each):
            raise ContainerError("plain bytes have no element size: give the width")
    else:
        each = list(widths) if isinstance(widths, (list, tuple, np.ndarray)) else [widths] * len(sources)
        if len(each) != len(sources):
            raise ContainerError("one width per item")
    if any(type(w) not in (int, np.uint8, np.int64, np.int32) or int(w) not in ITEM_WIDTHS for w in each):
        raise ContainerError(f"an element is 1, 2, 4 or 8 bytes wide, not {each!r}")
    w = np.array(each, dtype=np.uint8)
    preds, auto = _item_predictors(predict, w)
    parts = [x for x, _ in sources]
    lengths = np.array([int(x.numel()) if hasattr(x, "numel") else len(x) for x in parts], dtype=np.uint64)
    if int(lengths.sum()) == 0:
        return _pack_typed_items_device(ctx, None, lengths, w, preds, auto, coder, checksum, directory)
    return _pack_typed_items_device(ctx, _gather_device(parts), lengths, w, preds, auto, coder, checksum, directory)


def _unpack_typed_items_device(ctx, c, pick, verify: bool):
    """The picked items of a parsed RCXJ container, decoded, verified and joined on the device -> (the device buffer, the
    table of where each pick lies in it).  Only the picks' sub-items are decoded and checked."""
    import torch
    from . import rcx, typed_items
    pick = np.asarray(pick, dtype=np.int64)
    widths, preds = c["widths"][pick], c["preds"][pick]
    doffs = rcx.item_offsets(c["lengths"][pick])
    n = int(doffs[-1])
    d_out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    if n == 0:
        return d_out, doffs
    # the picks' sub-items, in order: back to back they are the split text of the picks back to back
    subs = np.concatenate([np.arange(c["sub_first"][k], c["sub_first"][k + 1], dtype=np.int64) for k in pick])
    owner = np.repeat(pick, widths.astype(np.int64))
    soffs = typed_items.sub_offsets(doffs, widths)
    d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.decode_items_device(_cuda(c["payload"]), len(c["payload"]), _cuda(c["offsets"]), soffs, d_split, pick=subs.astype(np.uint64), coder=c["coder"])
    ctx.sync_status()
    if verify and c["crcs"] is not None:
        ctx.verify_items_device(d_split, soffs, _cuda(c["crcs"][subs]))
        _sync_checked(ctx, "item", lambda k: int(owner[k]))
    typed_items.join_device(ctx, d_split, doffs, widths, preds, d_out)
    return d_out, doffs


def unpack_typed_items(blob, pick=None, ctx=None, verify: bool = True) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None); picks may repeat or be empty.  Only the
    picked items' sub-items are decoded, and in a container with checksums only they are verified: a mismatch raises
    ChecksumError naming the item."""
    from . import rcx
    c = parse_typed_items(blob)
    if pick is not None and any(not 0 <= int(k) < c["nitems"] for k in pick):
        raise ContainerError("no such item")
    picked = np.arange(c["nitems"], dtype=np.int64) if pick is None else np.array([int(k) for k in pick], dtype=np.int64)
    if len(picked) == 0:
        return []
    if int(c["lengths"][picked].sum()) == 0:
        return [b""] * len(picked)
    own = ctx is None
    ctx = ctx or rcx.Context(0)
    try:
        d_out, doffs = _unpack_typed_items_device(ctx, c, picked, verify)
        out = d_out.cpu().numpy()
        return [out[int(doffs[k]): int(doffs[k + 1])].tobytes() for k in range(len(picked))]
    finally:
        if own:
            ctx.close()


# ---- tensors with names, on top of the typed item container ---------------------------------------------------------------
def tensor_directory_bytes(entries) -> bytes:
    """entries: a list of dict(name, dtype, shape, first, count) -> the JSON directory of pack_tensors."""
    import json
    return json.dumps([{"name": str(e["name"]), "dtype": str(e["dtype"]), "shape": [int(d) for d in e["shape"]], "first": int(e["first"]),
                        "count": int(e["count"])} for e in entries], separators=(",", ":")).encode()


def parse_tensor_directory(directory: bytes, nitems: int) -> list:
    import json
    try:
        entries = json.loads(bytes(directory).decode())
        if not isinstance(entries, list):
            raise TypeError("not a list")
        out = [{"name": str(e["name"]), "dtype": str(e["dtype"]), "shape": tuple(int(d) for d in e["shape"]), "first": int(e["first"]),
                "count": int(e["count"])} for e in entries]
    except (ValueError, KeyError, TypeError) as err:
        raise ContainerError("the directory is not a tensor directory") from err
    if any(e["first"] < 0 or e["count"] < 0 or e["first"] + e["count"] > nitems or any(d < 0 for d in e["shape"]) for e in out):
        raise ContainerError("the directory names items the container does not have")
    if len({e["name"] for e in out}) != len(out):
        raise ContainerError("a name occurs twice in the directory")
    return out


def pack_tensors(named, block: int = 65536, predict=None, coder: int = 0, ctx=None, checksum: bool = False) -> bytes:
    """named: a dict of names -> numpy arrays or contiguous torch tensors (CPU or GPU) -> an RCXJ container whose directory
    names them.  Every tensor is cut into typed items of element_size * block bytes, its superblocks.  predict: None, a
    name or "auto" for all tensors, or a dict of names -> those (a name it lacks: none); tensors of 1-byte elements are never
    predicted.  An element size outside 1, 2, 4, 8 raises ContainerError."""
    import torch
    if not 16 <= block <= MAX_ITEM:
        raise ContainerError("a block is 16 bytes to RCX_MAX_BLOCK")
    parts, lengths, widths, entry_preds, entries = [], [], [], [], []
    for name, t in named.items():
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t if t.flags.c_contiguous else np.ascontiguousarray(t))
        if type(t).__module__.split(".")[0] != "torch":
            raise ContainerError(f"{name!r} is neither a numpy array nor a torch tensor")
        src, width = _item_source(t)
        if width not in ITEM_WIDTHS:
            raise ContainerError(f"{name!r}: an element is 1, 2, 4 or 8 bytes wide, not {width}")
        nbytes = int(src.numel()) if hasattr(src, "numel") else len(src)
        count = -(-nbytes // (width * block))
        entries.append({"name": name, "dtype": str(t.dtype).replace("torch.", ""), "shape": tuple(t.shape), "first": len(lengths), "count": count})
        each = predict.get(name) if isinstance(predict, dict) else predict
        if nbytes:
            parts.append(src)
            lengths += [width * block] * (count - 1) + [nbytes - (count - 1) * width * block]
            widths += [width] * count
            entry_preds += [None if width == 1 else each] * count
    w = np.array(widths, dtype=np.uint8)
    preds, auto = _item_predictors(entry_preds, w)
    lengths = np.array(lengths, dtype=np.uint64)
    directory = tensor_directory_bytes(entries)
    d_src = _gather_device(parts) if int(lengths.sum()) else None
    return _pack_typed_items_device(ctx, d_src, lengths, w, preds, auto, coder, checksum, directory)


def unpack_tensors(blob, names=None, device: str = "cpu", ctx=None, verify: bool = True) -> dict:
    """-> a dict of torch tensors of the recorded dtype and shape, on `device` ("cuda": no download).  names: only those
    tensors, and only their items are decoded (and verified)."""
    import torch
    from . import rcx
    c = parse_typed_items(blob)
    entries = parse_tensor_directory(c["directory"], c["nitems"])
    by_name = {e["name"]: e for e in entries}
    wanted = [e["name"] for e in entries] if names is None else list(names)
    if any(n not in by_name for n in wanted):
        raise ContainerError("no such tensor")
    for n in wanted:
        if not isinstance(getattr(torch, by_name[n]["dtype"], None), torch.dtype):
            raise ContainerError(f"{by_name[n]['dtype']!r} is no torch dtype")
    pick = np.concatenate([np.arange(by_name[n]["first"], by_name[n]["first"] + by_name[n]["count"], dtype=np.int64) for n in wanted] + [np.zeros(0, np.int64)])
    out, at = {}, 0
    flat, doffs = None, rcx.item_offsets(c["lengths"][pick])
    if int(doffs[-1]):
        own = ctx is None
        ctx = ctx or rcx.Context(0)
        try:
            flat, _ = _unpack_typed_items_device(ctx, c, pick, verify)
            flat = flat if device == "cuda" else flat.cpu()
        finally:
            if own:
                ctx.close()
    for n in wanted:
        e = by_name[n]
        dtype = getattr(torch, e["dtype"])
        a, b = int(doffs[at]), int(doffs[at + e["count"]])
        at += e["count"]
        count = int(np.prod(e["shape"], dtype=np.int64)) if len(e["shape"]) else 1
        if b - a != count * torch.empty(0, dtype=dtype).element_size():
            raise ContainerError(f"{n!r}: the items do not hold the tensor the directory describes")
        if b == a:
            out[n] = torch.empty(e["shape"], dtype=dtype, device=device)
        else:  # (a copy: a tensor begins where the one before ends, at any alignment)
            out[n] = flat[a:b].clone().view(dtype).reshape(e["shape"])
    return out
