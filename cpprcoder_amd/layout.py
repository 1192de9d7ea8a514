"""The five on-disk layouts of cpprcoder_amd/container.py, and nothing else: header writers, parsers, the tensor directory.
Plain Python and numpy: no torch, no library, no GPU.  All integers little-endian.

The block container, one buffer cut into blocks of one size:
    0   4  magic  b"RCXB"
    4   1  version (1; 2 with checksums; 3 with stored blocks)
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
Without checksums a container is byte for byte what it always was, version 1.

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
Without a predictor a container is byte for byte version 1.

Stored blocks (include/rcx_stored.h, cpprcoder_amd/stored.py): a block whose stream did not shrink is kept as its len_b raw
bytes.  Such a container is version 3 of either layout, and flag bit 2 (FLAG_STORED) is set; the two only ever appear together:
    RCXB version 3: the fixed part as above, flags bit 2 set (bits 0 and 1 as above); offsets; the bitmap; with bit 1 the CRC
        table; payload
    RCXT version 3: the fixed part as above, flags bit 2 set (bit 1 as above), byte 29 = the predictor, 0, 1 or 2; offsets;
        the bitmap; with bit 1 the CRC table; payload
    the bitmap: ceil(nblocks / 8) bytes, block b is bit b & 7 of byte b >> 3, padding bits zero, at least one bit set; a
        stored block's two offsets are len_b apart
The CRC stays the CRC of what the coder saw.  If no block ends up stored the container is, byte for byte, the one written
without the option.  An item container (RCXI) has no stored items and no version 3: a typed item of width 1 is a copy whose one
sub-item is the item, so the typed item container below, written with widths=1, IS the stored item container.

The typed item container holds many buffers of differing sizes, each with an element width (1, 2, 4 or 8) and a predictor
of its own (include/rcx_typed_items.h; cpprcoder_amd/typed_items.py): typed item i is transformed as one superblock of
m_i = len_i // w_i elements, and its w_i planes -- the last one with the len_i % w_i tail bytes -- are the coder's items, the
SUB-ITEMS, nsub = the sum of the widths; a sub-item of length 0 has no stream.  A fourth magic:
    0   4  magic  b"RCXJ"
    4   1  version (1; 2 with stored sub-items)
    5   1  coder
    6   2  flags: bit 1 = checksums (FLAG_CRC32); bit 2 = stored sub-items (FLAG_STORED: version 2, and only there); other bits 0
    8   8  nitems
    16  8  nsub
    24  8  dlen, the bytes of the directory
    32  8 * nitems      the items' lengths
    ..  nitems          their widths
    ..  nitems          their predictors (include/rcx_predict.h: 0 none, 1 delta, 2 delta + zigzag; 0 with width 1)
    ..  8 * (nsub + 1)  offsets of the sub-item streams in the payload
    ..  version 2: ceil(nsub / 8)  the bitmap of the stored sub-items, in the format above: sub-item s is bit s & 7 of byte
        s >> 3, padding bits zero, at least one bit set
    ..  with bit 1: 4 * nsub  the CRC-32 of each sub-item of the SPLIT text (0 for an empty one)
    ..  dlen            the directory: the caller's bytes, carried and not interpreted (may be empty)
    ..  payload: the sub-item streams back to back
Stored sub-items (include/rcx_stored_items.h, cpprcoder_amd/stored_items.py): a sub-item whose stream did not shrink is kept as
its raw bytes of the split text, its two offsets exactly its length apart; an empty sub-item is never stored.  Version 2 and
bit 2 only ever appear together, and only if at least one sub-item is stored: else the container is, byte for byte, the one
written without the option.  The CRC stays the CRC of the split text.  The tensor directory of pack_tensors is JSON: a list of {"name", "dtype" (torch's name),
"shape", "first", "count"}, where the tensor is the typed items first .. first + count - 1.

The delta container holds one buffer of 1-, 2-, 4- or 8-byte elements as its residual against a BASE, a second buffer of the
same length that the reader holds as well (include/rcx_base.h; cpprcoder_amd/base.py): a prefix that names the transform and
guards the base, and behind it a complete container of the residual's split text, written by the header writers above.  A
fifth magic:
    0   4  magic  b"RCXD"
    4   1  version (1)
    5   1  op: how an element and the base's element make a residual (include/rcx_base.h: 0 xor, 1 sub, 2 sub + zigzag)
    6   1  width: bytes per element (1, 2, 4 or 8)
    7   1  flags: bit 0 = the base's CRC table follows (DELTA_FLAG_BASE_CRC); every other bit 0
    8   4  block size in bytes
    12  4  zero
    16  8  n
    24  with bit 0: 4 * ceil(n / block)  the CRC-32 of every `block` bytes of the BASE in source order (the last one ragged):
        the residual decodes correctly whatever the base is, so the inner checksums cannot catch a wrong base; this table can
    ..  the inner container, to the end of the blob: for width 2, 4 or 8 an RCXT of that width without a predictor, for width 1
        (no planes) an RCXB without block sort; n and block are the prefix's.  Whatever those carry -- checksums of the split
        text, stored blocks, any coder -- they carry here, and an RCXT reader that skips the prefix gets the residual.

The delta item container holds many buffers of differing sizes, each with an element width and EITHER a predictor OR a base op
against a base buffer of its own length that the reader holds as well, or neither (include/rcx_base_items.h;
cpprcoder_amd/base_items.py): a state dict against the one before it, tensor by tensor.  As with RCXD, a prefix that names
the ops and guards the bases, and behind it a complete typed item container of the split text.  A sixth magic:
    0   4  magic  b"RCXK"
    4   1  version (1)
    5   1  flags: bit 0 = the base CRC table follows (DELTA_ITEMS_FLAG_BASE_CRC); every other bit 0
    6   2  zero
    8   8  nitems
    16  nitems  the items' ops (include/rcx_base.h: 0 xor, 1 sub, 2 sub + zigzag; 0xFF = the item has no base)
    ..  with bit 0: 4 * nitems  the CRC-32 of every item's base, all of its bytes (0 for an item without an op or without bytes)
    ..  a complete RCXJ container, to the end of the blob: the same nitems, and predictor 0 wherever the op is not 0xFF.  The
        checksums of the split text, stored sub-items, any coder and the directory are its own; an RCXJ reader that skips the
        prefix gets the residuals of the items with an op and the data of the others.
The tensor directory of pack_tensors_delta is that of pack_tensors.
"""
import json
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
_TYPED_FIXED = struct.Struct("<4sBBHIQQB7s")
WIDTHS = (2, 4, 8)
TYPED_ITEMS_MAGIC = b"RCXJ"
TYPED_ITEMS_VERSION = 1
TYPED_ITEMS_VERSION_STORED = 2  # + the bitmap of the stored sub-items behind the offsets; always with FLAG_STORED
_TYPED_ITEMS_FIXED = struct.Struct("<4sBBHQQQ")
ITEM_WIDTHS = (1, 2, 4, 8)
DELTA_MAGIC = b"RCXD"
DELTA_VERSION = 1
DELTA_FLAG_BASE_CRC = 1  # the CRC table of the base follows the fixed part
BASE_OPS = {"xor": 0, "sub": 1, "subzz": 2}  # include/rcx_base.h: RCX_BASE_*
_DELTA_FIXED = struct.Struct("<4sBBBBI4sQ")
DELTA_ITEMS_MAGIC = b"RCXK"
DELTA_ITEMS_VERSION = 1
DELTA_ITEMS_FLAG_BASE_CRC = 1  # the CRC table of the items' bases follows the ops
BASE_OP_NONE = 0xFF  # include/rcx_base_items.h: RCX_BASE_NONE
_DELTA_ITEMS_FIXED = struct.Struct("<4sBB2sQ")


def coded_size(n: int, flags: int) -> int:
    """What the entropy coder is handed for n original bytes (blksort.h:426-431 if block-sorted)."""
    return n + 2 * (n // 32768) if flags & FLAG_BLKSORT else n


class ContainerError(ValueError):
    pass


class BaseMismatchError(ContainerError):
    """A base whose CRC-32 differs from the delta container's table: `index` is the first such block of `block` bytes of the
    base.  Raised before anything is decoded: against another base the residual would decode to wrong bytes and no error."""

    def __init__(self, index: int):
        self.index = int(index)
        super().__init__(f"the base is not the one the container was packed against: base block {self.index} differs")


class BaseItemMismatchError(BaseMismatchError):
    """The same for a delta item container: `index` is the first picked item whose base differs from the one it was packed
    against, `name` its tensor in a container of tensors (else None)."""

    def __init__(self, index: int, name=None):
        self.index, self.name = int(index), name
        ContainerError.__init__(self, f"the base of item {self.index}" + (f", tensor {name!r}," if name is not None else "")
                                + " is not the one the container was packed against")


class ChecksumError(ContainerError):
    """Decoded bytes whose CRC-32 differs from the container's: `index` is the first such block (RCXB) or item (RCXI),
    counted as the container counts them."""

    def __init__(self, kind: str, index: int):
        self.kind, self.index = kind, int(index)
        super().__init__(f"checksum mismatch in {kind} {self.index}")


def block_lengths(m: int, block: int) -> np.ndarray:
    """len_b of every block of m bytes cut into blocks of `block`: all whole but the last."""
    nblocks = (m + block - 1) // block
    lengths = np.full(nblocks, block, dtype=np.uint64)
    if nblocks:
        lengths[-1] = m - (nblocks - 1) * block
    return lengths


# ---- what the layouts share ----------------------------------------------------------------------------------------------------
class _Cursor:
    """A blob read from the front: the fixed part as `fields` (magic, version, coder, flags, ...), then one table after another;
    `at` is where the next begins."""

    def __init__(self, blob, fixed: struct.Struct, magic: bytes):
        self.buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        if len(self.buf) < fixed.size:
            raise ContainerError("shorter than a header")
        self.fields = fixed.unpack(bytes(self.buf[: fixed.size]))
        self.at = fixed.size
        if self.fields[0] != magic:
            raise ContainerError(f"not an {magic.decode()} container")
        if self.fields[2] not in (0, 1, 2, 3):
            raise ContainerError("unsupported container version, coder or flags")

    def need(self, size: int, what: str) -> None:
        if len(self.buf) < self.at + size:  # (Python integers: a count of 2^63 is merely too large)
            raise ContainerError(f"truncated {what}")

    def take(self, count: int, dtype, what: str) -> np.ndarray:
        """`count` entries of `dtype`, called `what` if they are not all there -> a copy in the native byte order."""
        dtype = np.dtype(dtype)
        self.need(count * dtype.itemsize, what)
        a = np.frombuffer(bytes(self.buf[self.at: self.at + count * dtype.itemsize]), dtype=dtype).astype(dtype.newbyteorder("="))
        self.at += count * dtype.itemsize
        return a

    def crcs(self, checked: bool, count: int):
        return self.take(count, "<u4", "checksum table") if checked else None

    def bitmap(self, nblocks: int, none: str = "version 3 without a stored block") -> np.ndarray:
        """-> stored bool[nblocks]"""
        bits = np.unpackbits(self.take((nblocks + 7) // 8, np.uint8, "bitmap"), bitorder="little")
        if bits[nblocks:].any():
            raise ContainerError("a padding bit of the bitmap is set")
        if not bits[:nblocks].any():
            raise ContainerError(none)
        return bits[:nblocks].astype(bool)

    def payload(self, offsets, lengths=None, what: str = "an item") -> np.ndarray:
        """The rest of the blob, which the offset table must describe; with `lengths`, a stream of length 0 if and only if
        an item of length 0."""
        sizes = np.diff(offsets.astype(np.int64))
        if offsets[0] != 0 or np.any(sizes < 0) or self.at + int(offsets[-1]) != len(self.buf):
            raise ContainerError("offset table does not match the payload")
        if lengths is not None and np.any((lengths == 0) != (sizes == 0)):
            raise ContainerError(f"{what} of length 0 has no stream, and only such {what}")
        return self.buf[self.at:]


def _with_crcs(flags: int, crcs, count: int, per: str = "block or item"):
    """-> (the flags, with the CRC bit if there are checksums; the CRC table)"""
    if crcs is None:
        return flags, b""
    crcs = np.ascontiguousarray(crcs, dtype="<u4")
    if len(crcs) != count:
        raise ContainerError(f"one checksum per {per}")
    return flags | FLAG_CRC32, crcs.tobytes()


def _version_and_flags(flags: int, crcs, count: int):
    """RCXB and RCXI: version 1 as it always was, version 2 = the CRC bit + the table -> (version, flags, table)."""
    if crcs is None and flags & FLAG_CRC32:
        raise ContainerError("the checksum flag needs the checksums")
    flags, table = _with_crcs(flags, crcs, count)
    return (VERSION_CRC if flags & FLAG_CRC32 else VERSION), flags, table


def _check_version(version: int, flags: int, known: int) -> bool:
    """-> whether a CRC table follows.  Version 1: exactly the flags it always had; version 2: only with the CRC bit."""
    if version == VERSION and not flags & ~known:
        return False
    if version == VERSION_CRC and flags & FLAG_CRC32 and not flags & ~(known | FLAG_CRC32):
        return True
    raise ContainerError("unsupported container version, coder or flags")


def _stored_must_fit(stored, offsets, m: int, block: int) -> None:
    """A stored block's stream is the block: its two offsets are len_b apart."""
    sizes = np.diff(np.asarray(offsets).astype(np.int64))
    if np.any(sizes[stored] != block_lengths(m, block).astype(np.int64)[stored]):
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


# ---- RCXB ----------------------------------------------------------------------------------------------------------------------
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
    cur = _Cursor(blob, _FIXED, MAGIC)
    _, version, coder, flags, block, n, nblocks = cur.fields
    if version == VERSION_STORED:  # always with its flag; bits 0 and 1 as in the versions before
        if not flags & FLAG_STORED or flags & ~(FLAG_BLKSORT | FLAG_CRC32 | FLAG_STORED):
            raise ContainerError("unsupported container version, coder or flags")
        checked = bool(flags & FLAG_CRC32)
    else:
        checked = _check_version(version, flags, FLAG_BLKSORT)
    if block < 16 or block > (1 << 24) - 256 or nblocks != (coded_size(n, flags) + block - 1) // block:
        raise ContainerError("inconsistent header")
    offsets = cur.take(nblocks + 1, "<u8", "offset table")
    stored = cur.bitmap(nblocks) if version == VERSION_STORED else None
    crcs = cur.crcs(checked, nblocks)
    payload = cur.payload(offsets)
    if stored is not None:
        _stored_must_fit(stored, offsets, coded_size(n, flags), block)
    return {"coder": coder, "flags": flags, "block": block, "n": n, "nblocks": nblocks, "offsets": offsets, "crcs": crcs, "stored": stored,
            "payload": payload}


# ---- RCXI ----------------------------------------------------------------------------------------------------------------------
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
    cur = _Cursor(blob, _ITEM_FIXED, ITEM_MAGIC)
    _, version, coder, flags, nitems = cur.fields
    checked = _check_version(version, flags, 0)
    lengths = cur.take(nitems, "<u8", "tables")
    offsets = cur.take(nitems + 1, "<u8", "tables")
    crcs = cur.crcs(checked, nitems)
    if nitems and int(lengths.max()) > MAX_ITEM:
        raise ContainerError("an item is longer than the coder takes")
    return {"coder": coder, "nitems": nitems, "lengths": lengths, "offsets": offsets, "crcs": crcs, "payload": cur.payload(offsets, lengths)}


# ---- RCXT ----------------------------------------------------------------------------------------------------------------------
def typed_header_bytes(coder: int, block: int, n: int, width: int, offsets, crcs=None, pred: int = 0, stored=None) -> bytes:
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    nblocks = len(offsets) - 1
    if width not in WIDTHS:
        raise ContainerError("an element is 2, 4 or 8 bytes wide")
    if type(pred) is not int or pred not in (0, 1, 2):
        raise ContainerError("a predictor is 0 (none), 1 (delta) or 2 (zigzag)")
    if nblocks != (n + block - 1) // block:
        raise ContainerError("offsets do not match n and the block size")
    flags, table = _with_crcs(0, crcs, nblocks)
    version = TYPED_VERSION_PRED if pred else TYPED_VERSION  # version 2 only with a predictor
    bitmap = _bitmap_bytes(stored, offsets, n, block)
    if bitmap:  # version 3 only with a stored block
        version, flags = TYPED_VERSION_STORED, flags | FLAG_STORED
    return (_TYPED_FIXED.pack(TYPED_MAGIC, version, coder, flags, block, n, nblocks, width, bytes([pred]) + bytes(6)) + offsets.tobytes() + bitmap
            + table)


def parse_typed(blob):
    """-> dict(coder, flags, block, n, nblocks, width, pred, offsets uint64[nblocks+1], crcs uint32[nblocks] or None, stored bool[nblocks]
    or None, payload uint8 view); pred is 0 for a version 1 container"""
    cur = _Cursor(blob, _TYPED_FIXED, TYPED_MAGIC)
    _, version, coder, flags, block, n, nblocks, width, reserved = cur.fields
    known = FLAG_CRC32 | (FLAG_STORED if version == TYPED_VERSION_STORED else 0)  # bit 2 in version 3, and always there
    if version not in (TYPED_VERSION, TYPED_VERSION_PRED, TYPED_VERSION_STORED) or flags & ~known or (version == TYPED_VERSION_STORED and not flags & FLAG_STORED):
        raise ContainerError("unsupported container version, coder or flags")
    pred = reserved[0]
    pred_ok = pred in (1, 2) if version == TYPED_VERSION_PRED else pred in (0, 1, 2) if version == TYPED_VERSION_STORED else pred == 0
    if width not in WIDTHS or reserved[1:] != bytes(6) or not pred_ok:
        raise ContainerError("an element is 2, 4 or 8 bytes wide, version 2 names its predictor, and the reserved bytes are zero")
    if block < 16 or block > (1 << 24) - 256 or nblocks != (n + block - 1) // block:
        raise ContainerError("inconsistent header")
    offsets = cur.take(nblocks + 1, "<u8", "offset table")
    stored = cur.bitmap(nblocks) if version == TYPED_VERSION_STORED else None
    crcs = cur.crcs(bool(flags & FLAG_CRC32), nblocks)
    payload = cur.payload(offsets)
    if stored is not None:
        _stored_must_fit(stored, offsets, n, block)
    return {"coder": coder, "flags": flags, "block": block, "n": n, "nblocks": nblocks, "width": width, "pred": pred, "offsets": offsets,
            "crcs": crcs, "stored": stored, "payload": payload}


# ---- RCXJ ----------------------------------------------------------------------------------------------------------------------
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


def _stored_subs_must_fit(stored, offsets, sub) -> None:
    """A stored sub-item's stream is the sub-item: its two offsets are its length apart, and it has bytes."""
    sizes = np.diff(np.asarray(offsets).astype(np.int64))
    if np.any(np.asarray(sub)[stored] == 0):
        raise ContainerError("an empty sub-item is never stored")
    if np.any(sizes[stored] != np.asarray(sub).astype(np.int64)[stored]):
        raise ContainerError("a stored sub-item is not as long as its bytes")


def typed_items_header_bytes(coder: int, lengths, widths, preds, offsets, crcs=None, directory: bytes = b"", stored=None) -> bytes:
    """stored: one flag per sub-item, or None; version 2 if one is set, else the header without the option."""
    lengths, widths, preds, sub = _typed_items_tables(lengths, widths, preds)
    offsets = np.ascontiguousarray(offsets, dtype="<u8")
    if len(offsets) != len(sub) + 1:
        raise ContainerError("offsets do not match the number of sub-items")
    flags, table = _with_crcs(0, crcs, len(sub), "sub-item")
    version, bitmap = TYPED_ITEMS_VERSION, b""
    if stored is not None:
        stored = np.asarray(stored) != 0
        if len(stored) != len(sub):
            raise ContainerError("one stored flag per sub-item")
        if stored.any():
            _stored_subs_must_fit(stored, offsets, sub)
            version, flags, bitmap = TYPED_ITEMS_VERSION_STORED, flags | FLAG_STORED, np.packbits(stored, bitorder="little").tobytes()
    directory = bytes(directory)
    return (_TYPED_ITEMS_FIXED.pack(TYPED_ITEMS_MAGIC, version, coder, flags, len(lengths), len(sub), len(directory)) + lengths.tobytes()
            + widths.tobytes() + preds.tobytes() + offsets.tobytes() + bitmap + table + directory)


def parse_typed_items(blob):
    """-> dict(coder, flags, nitems, nsub, lengths uint64[nitems], widths uint8[nitems], preds uint8[nitems], sub_first int64[nitems + 1],
    sub_lengths uint64[nsub], offsets uint64[nsub + 1], crcs uint32[nsub] or None, directory bytes, payload uint8 view); a
    version 2 container has one key more, stored bool[nsub] -- .get("stored") is None for version 1, whose result is what it always was"""
    cur = _Cursor(blob, _TYPED_ITEMS_FIXED, TYPED_ITEMS_MAGIC)
    _, version, coder, flags, nitems, nsub, dlen = cur.fields
    has_bitmap = version == TYPED_ITEMS_VERSION_STORED  # bit 2 in version 2, and always there
    if version not in (TYPED_ITEMS_VERSION, TYPED_ITEMS_VERSION_STORED) or flags & ~(FLAG_CRC32 | (FLAG_STORED if has_bitmap else 0)) or (
            has_bitmap and not flags & FLAG_STORED):
        raise ContainerError("unsupported container version, coder or flags")
    if dlen > len(cur.buf):
        raise ContainerError("truncated tables")
    cur.need(10 * nitems + 8 * (nsub + 1), "tables")  # (all of them, before what they hold is looked at)
    lengths = cur.take(nitems, "<u8", "tables")
    widths = cur.take(nitems, np.uint8, "tables")
    preds = cur.take(nitems, np.uint8, "tables")
    _, _, _, sub = _typed_items_tables(lengths, widths, preds)  # (refuses bad widths and predictors, and sub-items that are too long)
    if len(sub) != nsub:
        raise ContainerError("the widths do not add up to the number of sub-items")
    offsets = cur.take(nsub + 1, "<u8", "tables")
    stored = cur.bitmap(nsub, "version 2 without a stored sub-item") if has_bitmap else None
    crcs = cur.crcs(bool(flags & FLAG_CRC32), nsub)
    directory = bytes(cur.take(dlen, np.uint8, "directory"))
    payload = cur.payload(offsets, sub, "a sub-item")
    if stored is not None:
        _stored_subs_must_fit(stored, offsets, sub)
    sub_first = np.concatenate([[0], np.cumsum(widths.astype(np.int64))])
    out = {"coder": coder, "flags": flags, "nitems": nitems, "nsub": nsub, "lengths": lengths, "widths": widths, "preds": preds, "sub_first": sub_first,
           "sub_lengths": sub.astype(np.uint64), "offsets": offsets, "crcs": crcs, "directory": directory, "payload": payload}
    if stored is not None:  # (a version 1 container parses to exactly what it always did: read the key with .get("stored"))
        out["stored"] = stored
    return out


# ---- RCXD ----------------------------------------------------------------------------------------------------------------------
def delta_header_bytes(op: int, width: int, block: int, n: int, base_crcs=None) -> bytes:
    """The prefix of a delta container; the inner container (typed_header_bytes with the same n, block and width and no
    predictor, or header_bytes without block sort for width 1, and its payload) follows it.  base_crcs: the CRC-32 of every
    `block` bytes of the base, or None for a container without that guard."""
    if type(op) is not int or op not in BASE_OPS.values():
        raise ContainerError("an op is 0 (xor), 1 (sub) or 2 (subzz)")
    if width not in ITEM_WIDTHS:
        raise ContainerError("an element is 1, 2, 4 or 8 bytes wide")
    if block < 16 or block > (1 << 24) - 256 or n < 0:
        raise ContainerError("inconsistent header")
    flags, table = 0, b""
    if base_crcs is not None:
        base_crcs = np.ascontiguousarray(base_crcs, dtype="<u4")
        if len(base_crcs) != (n + block - 1) // block:
            raise ContainerError("one checksum per block of the base")
        flags, table = DELTA_FLAG_BASE_CRC, base_crcs.tobytes()
    return _DELTA_FIXED.pack(DELTA_MAGIC, DELTA_VERSION, op, width, flags, block, bytes(4), n) + table


def parse_delta(blob):
    """-> dict(op, width, flags, block, n, base_crcs uint32[ceil(n / block)] or None, kind "typed" or "blocks", inner: what
    parse_typed or parse makes of the inner container, inner_at: where it begins in the blob)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _DELTA_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, op, width, flags, block, reserved, n = _DELTA_FIXED.unpack(bytes(buf[: _DELTA_FIXED.size]))
    if magic != DELTA_MAGIC:
        raise ContainerError("not an RCXD container")
    if version != DELTA_VERSION or op not in BASE_OPS.values() or flags & ~DELTA_FLAG_BASE_CRC:
        raise ContainerError("unsupported container version, op or flags")
    if width not in ITEM_WIDTHS or reserved != bytes(4):
        raise ContainerError("an element is 1, 2, 4 or 8 bytes wide, and the reserved bytes are zero")
    if block < 16 or block > (1 << 24) - 256:
        raise ContainerError("inconsistent header")
    at, base_crcs = _DELTA_FIXED.size, None
    if flags & DELTA_FLAG_BASE_CRC:
        size = 4 * ((n + block - 1) // block)
        if len(buf) < at + size:  # (Python integers: a count of 2^63 is merely too large)
            raise ContainerError("truncated checksum table of the base")
        base_crcs = np.frombuffer(bytes(buf[at: at + size]), dtype="<u4").astype(np.uint32)
        at += size
    rest = buf[at:]
    if width == 1:
        if bytes(rest[:4]) != MAGIC:
            raise ContainerError("the residual of 1-byte elements lies in an RCXB container")
        inner = parse(rest)
        if inner["flags"] & FLAG_BLKSORT:
            raise ContainerError("the residual is never block-sorted")
    else:
        if bytes(rest[:4]) != TYPED_MAGIC:
            raise ContainerError("the residual of 2-, 4- or 8-byte elements lies in an RCXT container")
        inner = parse_typed(rest)
        if inner["pred"] != 0:
            raise ContainerError("the residual takes no predictor")
        if inner["width"] != width:
            raise ContainerError("the inner container disagrees with the prefix")
    if inner["n"] != n or inner["block"] != block:
        raise ContainerError("the inner container disagrees with the prefix")
    return {"op": op, "width": width, "flags": flags, "block": block, "n": n, "base_crcs": base_crcs, "kind": "blocks" if width == 1 else "typed",
            "inner": inner, "inner_at": at}


# ---- RCXK ----------------------------------------------------------------------------------------------------------------------
def _delta_items_ops(ops) -> np.ndarray:
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    if np.any(~np.isin(ops, tuple(BASE_OPS.values()) + (BASE_OP_NONE,))):
        raise ContainerError("an op is 0 (xor), 1 (sub), 2 (subzz) or 0xFF (no base)")
    return ops


def delta_items_header_bytes(ops, base_crcs=None) -> bytes:
    """The prefix of a delta item container; the inner container (typed_items_header_bytes with one item per op, predictor 0
    wherever the op is not BASE_OP_NONE, and its payload) follows it.  base_crcs: the CRC-32 of every item's base (0 for an item
    without an op or without bytes), or None for a container without that guard."""
    ops = _delta_items_ops(ops)
    flags, table = 0, b""
    if base_crcs is not None:
        base_crcs = np.ascontiguousarray(base_crcs, dtype="<u4")
        if len(base_crcs) != len(ops):
            raise ContainerError("one checksum per item's base")
        if np.any(base_crcs[ops == BASE_OP_NONE] != 0):
            raise ContainerError("an item without a base has checksum 0")
        flags, table = DELTA_ITEMS_FLAG_BASE_CRC, base_crcs.tobytes()
    return _DELTA_ITEMS_FIXED.pack(DELTA_ITEMS_MAGIC, DELTA_ITEMS_VERSION, flags, bytes(2), len(ops)) + ops.tobytes() + table


def parse_delta_items(blob):
    """-> dict(flags, nitems, ops uint8[nitems], base_crcs uint32[nitems] or None, inner: what parse_typed_items makes of the inner
    container, inner_at: where it begins in the blob)"""
    buf = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    if len(buf) < _DELTA_ITEMS_FIXED.size:
        raise ContainerError("shorter than a header")
    magic, version, flags, reserved, nitems = _DELTA_ITEMS_FIXED.unpack(bytes(buf[: _DELTA_ITEMS_FIXED.size]))
    if magic != DELTA_ITEMS_MAGIC:
        raise ContainerError("not an RCXK container")
    if version != DELTA_ITEMS_VERSION or flags & ~DELTA_ITEMS_FLAG_BASE_CRC:
        raise ContainerError("unsupported container version or flags")
    if reserved != bytes(2):
        raise ContainerError("the reserved bytes are zero")
    at, base_crcs = _DELTA_ITEMS_FIXED.size, None
    size = nitems * (5 if flags & DELTA_ITEMS_FLAG_BASE_CRC else 1)
    if len(buf) < at + size:  # (Python integers: a count of 2^63 is merely too large)
        raise ContainerError("truncated tables of the ops and the bases")
    ops = _delta_items_ops(np.array(buf[at: at + nitems]))
    at += nitems
    if flags & DELTA_ITEMS_FLAG_BASE_CRC:
        base_crcs = np.frombuffer(bytes(buf[at: at + 4 * nitems]), dtype="<u4").astype(np.uint32)
        at += 4 * nitems
    rest = buf[at:]
    if bytes(rest[:4]) != TYPED_ITEMS_MAGIC:
        raise ContainerError("the split text lies in an RCXJ container")
    inner = parse_typed_items(rest)
    if inner["nitems"] != nitems:
        raise ContainerError("the inner container disagrees with the prefix")
    if np.any((ops != BASE_OP_NONE) & (inner["preds"] != 0)):
        raise ContainerError("an item with a base takes no predictor")
    return {"flags": flags, "nitems": nitems, "ops": ops, "base_crcs": base_crcs, "inner": inner, "inner_at": at}


# ---- the tensor directory ------------------------------------------------------------------------------------------------------
def tensor_directory_bytes(entries) -> bytes:
    """entries: a list of dict(name, dtype, shape, first, count) -> the JSON directory of pack_tensors."""
    return json.dumps([{"name": str(e["name"]), "dtype": str(e["dtype"]), "shape": [int(d) for d in e["shape"]], "first": int(e["first"]),
                        "count": int(e["count"])} for e in entries], separators=(",", ":")).encode()


def parse_tensor_directory(directory: bytes, nitems: int) -> list:
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
