"""A file container around the many-block coder ("multi-block container"; 8(f) row 3): pack and unpack.

The reference has no multi-block format (one stream per file, test/main.cpp:304-364); this is the framing the
block engine needs to be usable on files.  Every block's stream inside is bit-exact what the reference's
AdaptiveRangeEncoder (or RangeEncoder, coder = 1; rANS::encode, coder = 2; rANS::encode_simd, coder = 3) emits
for that block, so a reader with only the reference can decode a container block by block.

The five layouts -- RCXB blocks, RCXI items, RCXT typed blocks, RCXJ typed items, RCXD residuals -- their header writers and parsers are
cpprcoder_amd/layout.py, plain Python, and every public name of it is a name of this module too.  pack()/unpack() and
their kin here go through the HIP library (there is no CPU coder: without librcx.so and a GPU they raise), except where there
is nothing to code or decode.

Checksums are opt-in (pack(..., checksum=True)).  The decoders cannot tell that a damaged payload came back wrong
(include/rcx.h, "Damaged streams": it still decodes to some bytes); with checksums unpack(), unpack_range() and
unpack_items() compare what they decoded, on the GPU, before they hand it back, and raise ChecksumError naming the first bad
block or item (verify=False skips that).  The checked paths upload once and use the device calls (encode + CRC, decode +
verify): they give up the overlap of copies and kernels that the host-buffer calls have.

unpack_range(blob, start, stop) decodes only the blocks that cover [start, stop), through the item call
(rcx_decode_items: any subset of a set of streams).  It is refused for block-sorted containers, whose bytes are
not in place before the whole inverse transform has run.

unpack_typed_range(blob, start, stop) decodes the blocks of the superblocks that cover [start, stop) and joins that span
as a buffer of its own: the transform of a span from one superblock border to another, or to n, is the transform of the
span taken alone.  A predictor (pack_typed(..., predict="delta" | "zigzag"): for integers whose differences are small) is
opt-in and restarts in every superblock, so all of that holds with it.

Stored blocks (pack(..., stored=True | fraction), pack_typed(..., stored=...); include/rcx_stored.h, cpprcoder_amd/stored.py): a
block whose stream did not shrink -- coded_b + floor(len_b * gain / 65536) >= len_b, gain = 0 for True, min(65535, int(g * 65536))
for a fraction 0 <= g < 1 -- is kept as its len_b raw bytes and decoded by copy, so a payload never exceeds what the coder
saw.  With the option the pack path is the device path of the checked containers: one upload, encode, mix (and CRC), one
download.

pack_typed(..., predict="auto") measures instead of asking (include/rcx_stats.h; cpprcoder_amd/stats.py).  For each of none,
delta and zigzag the split text's order-0 cost is C_p = the sum of the blocks' costs -- what an order-0 coder with one model a
block will make of it, to within a few percent.  The rule (pick_predictor): a predictor is a candidate only if it earns at
least 1/64, 64 * C_p < 63 * C_none; the cheaper candidate is taken, delta on a tie; without a candidate, none.  The margin
keeps data that no predictor helps on version 1: uniform bytes at 4 KiB blocks would otherwise take delta for 0.002 %.  The
container is byte for byte what predict=<the choice> writes, and nothing in it records that the choice was measured.

unpack_typed_items(blob, pick) decodes the picked items' sub-items and no others, verifies those, and joins them as a call of
its own with re-based offsets: every item is a superblock of its own, so any subset is exact.  predict="auto" decides PER
ITEM with pick_predictor on the sum of its sub-items' order-0 costs under the three candidates.  There is no command-line
subcommand.  pack_tensors / unpack_tensors put tensors with names on top of it and nothing else: every tensor is cut into
typed items of element_size * block bytes -- its superblocks, so its sub-items are the blocks pack_typed would code -- and the
directory names them (layout.py).

Stored sub-items (pack_typed_items(..., stored=...), pack_tensors(..., stored=...); include/rcx_stored_items.h,
cpprcoder_amd/stored_items.py): the same option with the sub-item in the block's place -- the mix runs behind the item encode call,
an empty sub-item is never stored, and unpack goes through the decode call that copies.  The container is RCXJ version 2 if a
sub-item ends up stored, else byte for byte the one written without the option.  RCXI has no such version:
pack_typed_items(items, widths=1, stored=True) is the stored item container.

Residuals against a base (pack_delta(data, base, ...); include/rcx_base.h, cpprcoder_amd/base.py): for a buffer that differs a
little from one the reader already has -- a checkpoint against the one before, a fine-tuned model against its base model, a
counter table against its last snapshot.  Every element becomes its residual against the base's element at the same place
(op="xor", "sub" or "subzz", the zigzagged difference), and the residuals' split text is coded as pack_typed codes it (width 1:
as pack codes it), so checksum=, stored= and every coder come with it.  The container is RCXD: a prefix and that inner container
(layout.py).  Against an unrelated base the payload grows by some 5 %, so the option is never chosen for the caller.  The
residual decodes correctly whatever the base is, so the inner checksums cannot catch a wrong base: with base_check (the
default) the prefix carries the CRC-32 of every block of the base, and unpack_delta and unpack_delta_range verify the base they
are given against it, on the device, before anything is decoded -- BaseMismatchError names the first bad block of the base.
unpack_delta_range decodes the blocks of the superblocks that cover the range, verifies only those blocks of the base and joins
the span against the same span of the base: the transform is elementwise.  Not here: tensors by name against a base
(pack_tensors), chains of deltas, bases of another length.

Residuals against a base per item (pack_delta_items(items, bases, ...), pack_tensors_delta(named, base, ...);
include/rcx_base_items.h, cpprcoder_amd/base_items.py): tensors by name against a base ARE here.  Every item has a width and
either a predictor, or an op against a base of its own length, or neither; one split call transforms them all, and the
sub-items are coded as pack_typed_items codes them.  The container is RCXK: a prefix with the items' ops and, with base_check
(the default), the CRC-32 of every item's base, then a complete RCXJ (layout.py).  unpack_delta_items and unpack_tensors_delta
need only the picked items' bases and verify them on the device before anything is decoded: BaseItemMismatchError names the
item and, for tensors, the tensor.  pack_tensors_delta gives a tensor the op if the base holds its name with the same dtype
and shape, and packs every other tensor as pack_tensors does.

"auto" for ops (pack_delta_items(ops=[..., "auto", ...]), pack_tensors_delta(op="auto"), pack_delta(op="auto"); include/rcx_typed_stats.h,
cpprcoder_amd/typed_stats.py): which of xor, sub and subzz an item wants, or whether it wants its base at all, is measured: one
call reads items and bases once and gives the order-0 cost of every asked candidate -- none, delta, zigzag, xor, sub, subzz -- of
every item, exactly what the split and statistics calls give one candidate at a time.  The rule (pick_candidate) is the one
of predict="auto", extended: a candidate other than none qualifies if 64 * C < 63 * C_none; the cheapest qualifying one wins;
ties go in the order delta, zigzag, subzz, sub, xor -- what needs no base first, subzz the default among the ops; if nothing
qualifies the item is packed without its base and without a predictor.  An "auto" item is measured under none and the three ops,
with predict="auto" under all six; pack_tensors_delta decides per tensor on the sums over its items, so a tensor needs its
base entirely or not at all; pack_delta decides among the three ops only (pick_op: cheapest, ties subzz, sub, xor, no margin),
because RCXD cannot say "no base".  The container is byte for byte what the decided names given explicitly write, and nothing in
it records that they were measured; choose_delta_items and choose_tensors_delta return the decision alone, their
_from_costs siblings make it from a table without a GPU.

open_items(blob) (include/rcx_picks.h, cpprcoder_amd/picks.py) is for a reader that picks on the GPU: an RCXI container, or the
stored item container, is parsed once and its payload, stream table, stored flags and lengths are put on the device; decode_into
takes picks, destinations and their count from device tensors, only enqueues, and can be captured in a graph and replayed
against tables that device code rewrites.  A bad entry is skipped and latched (sync_status), every other entry decodes.
open_typed_items(blob) does the same for an RCXJ container with the typed join behind the decode (include/rcx_typed_picks.h),
and open_delta_items(blob, bases) (cpprcoder_amd/delta_open.py, reached as container.open_delta_items) for an RCXK container with
the join against the bases (include/rcx_base_picks.h, cpprcoder_amd/base_picks.py): the bases are gathered into one device buffer once, the same object given for many items is one
span, and the prefix's CRC-32 guard is checked at open.

pack_items_device(ctx, d_src, d_src_at, d_src_len, d_count, max_items, max_len, max_bytes) (include/rcx_encode_picks.h;
cpprcoder_amd/encode_picks.py, reached as container.pack_items_device) is the way in for a writer that picks on the GPU: the items'
positions, lengths and count are device tensors, the call enqueues the encode and returns a PackedItems over the device-resident
streams without a download or a synchronisation; its decode_into is open_items' decode_into, its to_bytes() the RCXI file that
pack_items writes for the same items (no checksums).  pack_typed_items_device(ctx, d_src, d_src_at, d_len, d_widths, d_preds,
d_count, max_items, max_len, max_bytes) (include/rcx_typed_split_picks.h; cpprcoder_amd/typed_split_picks.py, reached as
container.pack_typed_items_device) is the same for typed items: the device-planned split into a staging buffer in front of that
encode, a width and a predictor per item read on the device; its PackedTypedItems decodes and joins with open_typed_items'
decode_into, and its to_bytes() is the RCXJ file that pack_typed_items writes for the same items (no checksums).
"""
import collections
import contextlib

import numpy as np

from .layout import (BASE_OP_NONE, BASE_OPS, DELTA_FLAG_BASE_CRC, DELTA_ITEMS_FLAG_BASE_CRC, DELTA_ITEMS_MAGIC, DELTA_ITEMS_VERSION, DELTA_MAGIC,  # noqa: F401
                     DELTA_VERSION, FLAG_BLKSORT, FLAG_CRC32, FLAG_STORED, ITEM_MAGIC, ITEM_VERSION,
                     ITEM_WIDTHS, MAGIC, MAX_ITEM, PREDICTORS,
                     TYPED_ITEMS_MAGIC, TYPED_ITEMS_VERSION, TYPED_ITEMS_VERSION_STORED, TYPED_MAGIC, TYPED_VERSION, TYPED_VERSION_PRED, TYPED_VERSION_STORED, VERSION,
                     VERSION_CRC, VERSION_STORED, WIDTHS, BaseItemMismatchError, BaseMismatchError, ChecksumError, ContainerError, _typed_items_tables,
                     block_lengths, coded_size, delta_header_bytes, delta_items_header_bytes, header_bytes, item_header_bytes, parse, parse_delta,
                     parse_delta_items, parse_items, parse_tensor_directory, parse_typed, parse_typed_items, tensor_directory_bytes, typed_header_bytes,
                     typed_items_header_bytes)

AUTO = "auto"  # pack_typed(predict=AUTO): measured, see pick_predictor; never in a container


@contextlib.contextmanager
def _scope(ctx):
    """The caller's context, or one of this call's own, closed behind it."""
    if ctx is not None:
        yield ctx
        return
    from . import rcx
    own = rcx.Context(0)
    try:
        yield own
    finally:
        own.close()


def _source(data):
    """-> (the bytes: a uint8 cuda tensor if `data` lies on the GPU, else a uint8 numpy array; the element size, None for plain bytes)"""
    if type(data).__module__.split(".")[0] == "torch":
        import torch
        if not data.is_contiguous():
            raise ContainerError("a tensor must be contiguous")
        flat = data.detach().reshape(-1).view(torch.uint8)
        return (flat if flat.is_cuda else flat.numpy()), data.element_size()
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).reshape(-1).view(np.uint8), data.dtype.itemsize
    return np.frombuffer(data, dtype=np.uint8), None


def _size(src) -> int:
    return int(src.numel()) if hasattr(src, "numel") else len(src)


def _element_width(size, width, allowed, text: str) -> int:
    """width=None: the element size of the array or tensor; plain bytes need a width."""
    width = size if width is None else width
    if width is None:
        raise ContainerError("plain bytes have no element size: give the width")
    if width not in allowed:
        raise ContainerError(f"an element is {text} bytes wide, not {width}")
    return width


# ---- the device paths: one upload, the device calls, one download --------------------------------------------------------
def _cuda(a, dtype=None):
    import torch
    a = np.array(a, dtype=dtype)  # (a writable copy: a container's arrays are views of the caller's bytes)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _crcs_of(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).copy()


def _gain(stored):
    """The option stored=None | True | fraction of the pack calls -> None, or the gain of include/rcx_stored.h."""
    if stored is None or stored is False:
        return None
    from . import stored as calls
    try:
        return calls.gain_q16(stored)
    except ValueError as e:
        raise ContainerError(f"stored is None, True or a fraction 0 <= g < 1 of the block, not {stored!r}") from e


def _encode_device(ctx, d_src, cut, coder: int, checksum: bool, gain=None):
    """The coder's input on the device, cut into blocks (cut: the block size) or into items (cut: their table of offsets)
    -> (payload, offsets, crcs or None, stored flags or None): encode, the mix of the stored blocks or items behind it (with a
    gain: include/rcx_stored.h, rcx_stored_items.h), the CRC-32 of every block or item of d_src (if asked for), one sync, the
    downloads."""
    import torch
    from . import rcx, stored, stored_items
    items = np.ndim(cut) > 0
    count = len(cut) - 1 if items else rcx.block_count(d_src.numel(), cut)
    bound = max(rcx.encode_items_bound(cut, coder), 1) if items else rcx.encode_bound(d_src.numel(), cut, coder)
    d_dst = torch.empty(bound, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(count + 1, dtype=torch.int64, device="cuda")
    (ctx.encode_items_device if items else ctx.encode_blocks_device)(d_src, cut, d_dst, d_offs, coder=coder)
    d_flags = None
    if gain is not None:  # (a mixed payload is never longer than the text)
        d_mixed = torch.empty(max(int(cut[-1] - cut[0]) if items else d_src.numel(), 1), dtype=torch.uint8, device="cuda")
        d_moffs = torch.zeros(count + 1, dtype=torch.int64, device="cuda")
        d_flags = torch.zeros(max(count, 1), dtype=torch.uint8, device="cuda")
        (stored_items.mix_items_device if items else stored.mix_device)(ctx, d_src, cut, d_dst, d_dst.numel(), d_offs, gain, d_mixed, d_moffs, d_flags)
        d_dst, d_offs, d_flags = d_mixed, d_moffs, d_flags[:count]
    if checksum:
        d_crc = torch.zeros(count, dtype=torch.int32, device="cuda")
        (ctx.crc32_items_device if items else ctx.crc32_blocks_device)(d_src, cut, d_crc)
    ctx.sync_status()
    offsets = d_offs.cpu().numpy().astype(np.uint64)
    return (d_dst[: int(offsets[-1])].cpu().numpy(), offsets, _crcs_of(d_crc) if checksum else None,
            None if d_flags is None else d_flags.cpu().numpy())


def _raise_latched(ctx, mismatch, what: str) -> None:
    """The latch behind a verify call: a mismatch becomes the exception mismatch(position) makes, any other failure RcxError
    naming `what` and the position."""
    from . import rcx
    st, bad = ctx.sync_status(raise_on_error=False)
    if st == rcx.E_CORRUPT:
        raise mismatch(int(bad))
    if st != rcx.OK:
        raise rcx.RcxError(st, f"{what} {bad}")


def _verify_items_device(ctx, d_out, doffs, crcs, kind: str, owner) -> None:
    """Stream k of d_out at doffs against crcs[k] -> ChecksumError naming owner[k], the container's index of it."""
    ctx.verify_items_device(d_out, doffs, _cuda(crcs))
    _raise_latched(ctx, lambda k: ChecksumError(kind, int(owner[k])), kind)


def _decode_streams_device(ctx, c, doffs, d_out, pick=None) -> None:
    """The streams pick[k] of a parsed container -> d_out at doffs; pick=None: every block, d_out whole.  With stored streams
    through the call that copies them.  Then the sync: the decoder's own failures come first -- a stream that runs dry is an
    RcxError, as without checksums."""
    from . import stored
    d_payload, d_offsets = _cuda(c["payload"]), _cuda(c["offsets"])
    if c.get("stored") is not None:
        stored.decode_device(ctx, d_payload, len(c["payload"]), d_offsets, c["stored"], doffs, d_out, pick=pick, coder=c["coder"])
    elif pick is None:
        ctx.decode_blocks_device(d_payload, len(c["payload"]), d_offsets, d_out.numel(), c["block"], d_out, coder=c["coder"])
    else:
        ctx.decode_items_device(d_payload, len(c["payload"]), d_offsets, doffs, d_out, pick=pick, coder=c["coder"])
    ctx.sync_status()


def _decode_all_device(ctx, c, m: int, verify: bool):
    """Every block of a container, m bytes -> the device buffer; then, if `verify` and the container has checksums, the blocks
    are verified."""
    import torch
    d_out = torch.empty(m, dtype=torch.uint8, device="cuda")
    _decode_streams_device(ctx, c, np.minimum(np.arange(c["nblocks"] + 1, dtype=np.uint64) * np.uint64(c["block"]), np.uint64(m)), d_out)
    if verify and c["crcs"] is not None:
        ctx.verify_blocks_device(d_out, c["block"], _cuda(c["crcs"]))
        _raise_latched(ctx, lambda k: ChecksumError("block", k), "block")
    return d_out


def _decode_picked_device(ctx, c, lengths, pick, kind: str, checked: bool):
    """Streams pick[k] of a container, decoded back to back on the device and, if `checked`, verified there
    -> (the device buffer, the table of where each pick lies in it)."""
    import torch
    from . import rcx
    pick = np.asarray(pick, dtype=np.uint64)
    at = pick.astype(np.int64)
    doffs = rcx.item_offsets(np.asarray(lengths, dtype=np.uint64)[at])
    d_out = torch.empty(max(int(doffs[-1]), 1), dtype=torch.uint8, device="cuda")
    _decode_streams_device(ctx, c, doffs, d_out, pick)
    if checked:
        _verify_items_device(ctx, d_out, doffs, c["crcs"][at], kind, at)
    return d_out, doffs


# ---- RCXB and RCXI ---------------------------------------------------------------------------------------------------------------
def pack(data, block: int = 65536, coder: int = 0, ctx=None, blksort: bool = False, checksum: bool = False, stored=None) -> bytes:
    """stored=True | fraction: blocks that do not shrink (by that fraction of their length) are kept raw, see the module's
    docstring; the container is version 3 if there is such a block, else the one written without the option."""
    gain = _gain(stored)
    with _scope(ctx) as ctx:
        src = _source(data)[0]
        flags = FLAG_BLKSORT if blksort else 0
        if len(src) == 0:
            return header_bytes(coder, block, 0, np.zeros(1, np.uint64), flags, np.zeros(0, np.uint32) if checksum else None)
        if checksum or gain is not None:  # block sort (if asked for), encode, mix and CRC-32 of the coder's input, all on the device
            d_src = _cuda(src)
            if blksort:
                import torch
                from . import rcx
                d_sorted = torch.empty(rcx.bwt_encode_bound(len(src)), dtype=torch.uint8, device="cuda")
                ctx.bwt_encode_device(d_src, d_sorted)
                d_src = d_sorted[: coded_size(len(src), FLAG_BLKSORT)]
            payload, offsets, crcs, raw = _encode_device(ctx, d_src, block, coder, checksum, gain)
            return header_bytes(coder, block, len(src), offsets, flags, crcs, raw) + payload.tobytes()
        payload, offsets = ctx.encode_blocks(ctx.bwt_encode(src) if blksort else src, block, coder=coder)
        return header_bytes(coder, block, len(src), offsets, flags) + payload.tobytes()


def _unpack_device(ctx, c, verify: bool = True) -> bytes:
    import torch
    m = coded_size(c["n"], c["flags"])
    d_out = _decode_all_device(ctx, c, m, verify)
    if c["flags"] & FLAG_BLKSORT:
        d_text = torch.empty(max(c["n"], 1), dtype=torch.uint8, device="cuda")
        ctx.bwt_decode_device(d_out, m, d_text)
        ctx.sync_status()
        d_out = d_text[: c["n"]]
    return d_out.cpu().numpy().tobytes()


def unpack(blob, ctx=None, verify: bool = True) -> bytes:
    c = parse(blob)
    if c["n"] == 0:
        return b""
    with _scope(ctx) as ctx:
        if (verify and c["crcs"] is not None) or c["stored"] is not None:
            return _unpack_device(ctx, c, verify)
        m = coded_size(c["n"], c["flags"])
        out = ctx.decode_blocks(c["payload"], c["offsets"], c["block"], capacity=m, coder=c["coder"])
        if len(out) != m:
            raise ContainerError("decoded size differs from the header")
        if c["flags"] & FLAG_BLKSORT:
            out = ctx.bwt_decode(out)
        return out.tobytes()


def unpack_range(blob, start: int, stop: int, ctx=None, verify: bool = True) -> bytes:
    """The bytes [start, stop) of the original, decoding -- and, in a container with checksums, verifying -- only the
    blocks that cover them."""
    c = parse(blob)
    if c["flags"] & FLAG_BLKSORT:
        raise ContainerError("a block-sorted container has no byte ranges: unpack() it")
    if not 0 <= start <= stop <= c["n"]:
        raise ContainerError("range outside the data")
    if start == stop:
        return b""
    block = c["block"]
    first, last = start // block, (stop - 1) // block
    pick = np.arange(first, last + 1, dtype=np.uint64)
    lengths = block_lengths(c["n"], block)
    with _scope(ctx) as ctx:
        checked = verify and c["crcs"] is not None
        if checked or c["stored"] is not None:
            d_out, doffs = _decode_picked_device(ctx, c, lengths, pick, "block", checked)
            out = d_out[: int(doffs[-1])].cpu().numpy()
        else:
            out = np.concatenate(ctx.decode_items(c["payload"], c["offsets"], lengths, pick=pick, coder=c["coder"]))
    return out[start - first * block: stop - first * block].tobytes()


def pack_items(items, coder: int = 0, ctx=None, checksum: bool = False) -> bytes:
    """items: a list of buffers -> an RCXI container.  It has no stored items: pack_typed_items(items, widths=1, stored=...) is
    the stored item container (a typed item of width 1 is a copy whose one sub-item is the item), and never exceeds its items."""
    with _scope(ctx) as ctx:
        parts = [_source(x)[0] for x in items]
        lengths = [len(x) for x in parts]
        if checksum:
            from . import rcx
            d_src = _cuda(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
            payload, offsets, crcs, _ = _encode_device(ctx, d_src, rcx.item_offsets(lengths), coder, True)
            return item_header_bytes(coder, lengths, offsets, crcs) + payload.tobytes()
        payload, offsets = ctx.encode_items(parts, coder=coder)
        return item_header_bytes(coder, lengths, offsets) + payload.tobytes()


def unpack_items(blob, pick=None, ctx=None, verify: bool = True) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None); picks may repeat.  In a container
    with checksums the picked items, and only they, are verified."""
    c = parse_items(blob)
    if pick is not None and any(not 0 <= int(k) < c["nitems"] for k in pick):
        raise ContainerError("no such item")
    if c["nitems"] == 0 or (pick is not None and len(pick) == 0):
        return []
    with _scope(ctx) as ctx:
        if verify and c["crcs"] is not None:
            picked = np.arange(c["nitems"], dtype=np.uint64) if pick is None else pick
            d_out, doffs = _decode_picked_device(ctx, c, c["lengths"], picked, "item", True)
            out = d_out.cpu().numpy()
            return [out[int(doffs[k]): int(doffs[k + 1])].tobytes() for k in range(len(picked))]
        return [x.tobytes() for x in ctx.decode_items(c["payload"], c["offsets"], c["lengths"], pick=pick, coder=c["coder"])]


class _Opened:
    """What both have: the context (the caller's, or one of its own that close() closes) and, on the device, the payload, the
    stream table, the stored flags and the items' lengths."""

    def __init__(self, c, lengths, offsets, stored, crcs, ctx):
        import torch
        from . import picks, rcx
        self.coder, self.nitems = c["coder"], len(lengths)
        self.lengths = np.array(lengths, dtype=np.uint64)
        self.crcs = crcs
        self.max_len = int(self.lengths.max()) if self.nitems else 0
        self._own = ctx is None
        self.ctx = rcx.Context(0) if ctx is None else ctx
        self.payload_size = len(c["payload"])
        self.d_payload = torch.zeros(max(self.payload_size, 16), dtype=torch.uint8, device="cuda")
        if self.payload_size:
            self.d_payload[: self.payload_size] = _cuda(c["payload"])
        self.d_offsets = _cuda(offsets)
        self.d_stored = None if stored is None else _cuda(np.asarray(stored) != 0, dtype=np.uint8)
        self.d_lengths = _cuda(self.lengths if self.nitems else np.zeros(1, np.uint64))
        self._picks = picks

    def close(self) -> None:
        if self._own and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class OpenItems(_Opened):
    """An item container on the device (open_items): payload, stream table, stored flags and the items' lengths are uploaded
    once; decode_into enqueues one call whose picks, destinations and count are read on the device (include/rcx_picks.h)."""

    def reserve(self, max_pick: int) -> None:
        """The scratch of decode_into calls with at most max_pick entries: after it they allocate nothing in the context."""
        self._picks.reserve(self.ctx, max_pick, self.max_len, self.coder)

    def decode_into(self, d_pick, d_dst_at, d_count, d_dst, max_pick: int | None = None, stream=None) -> None:
        """Entry k < d_count[0]: item d_pick[k] -> d_dst[d_dst_at[k] : + its length].  d_pick, d_dst_at: int64 cuda tensors
        [>= max_pick]; d_count: an int64 cuda tensor of one entry; d_dst: a uint8 cuda tensor.  Enqueues only: the lengths are
        looked up on the device (an entry that names no item gets length 1, so that the call skips and latches it; entries at or
        past the count may hold anything).  Failures are the context's: sync_status()."""
        import torch
        max_pick = d_pick.numel() if max_pick is None else int(max_pick)
        p = d_pick[:max_pick]
        inside = (p >= 0) & (p < self.nitems)
        d_len = torch.where(inside, self.d_lengths[torch.clamp(p, 0, max(self.nitems - 1, 0))], torch.ones_like(p))
        self._picks.decode_device(self.ctx, self.d_payload, self.payload_size, self.d_offsets, p, d_dst_at, d_len, d_count, d_dst, self.max_len,
                                  max_pick=max_pick, stored=self.d_stored, coder=self.coder, stream=stream)

    def verify(self, d_out, pick, dst_offsets=None) -> None:
        """For a result that lies back to back (item pick[k] at dst_offsets[k], the prefix sums of the lengths if None): the
        CRC-32 check of a container with checksums, on the device -> ChecksumError naming the item.  pick is a HOST table."""
        if self.crcs is None:
            return
        from . import rcx
        pick = np.asarray(pick, dtype=np.int64)
        doffs = rcx.item_offsets(self.lengths[pick]) if dst_offsets is None else np.asarray(dst_offsets, dtype=np.uint64)
        _verify_items_device(self.ctx, d_out, doffs, self.crcs[pick], "item", pick)


def open_items(blob, ctx=None) -> OpenItems:
    """An item container -- RCXI (pack_items, with or without checksums) or the stored item container, RCXJ whose items all have
    width 1 (pack_typed_items(items, widths=1, stored=...)) -- parsed once and put on the device -> OpenItems, whose decode_into
    takes picks, destinations and their count from device memory and can be captured in a graph.  ctx=None: a context of its
    own, closed by close()."""
    head = bytes(memoryview(blob)[:4])
    if head == TYPED_ITEMS_MAGIC:
        c = parse_typed_items(blob)
        if np.any(c["widths"] != 1):
            raise ContainerError("open_items takes typed items of width 1 only: wider items are joined after they are decoded")
        return OpenItems(c, c["lengths"], c["offsets"], c.get("stored"), c["crcs"], ctx)
    c = parse_items(blob)
    return OpenItems(c, c["lengths"], c["offsets"], None, c["crcs"], ctx)


# ---- RCXT: the byte-plane filter in front of the coder -----------------------------------------------------------------------------
def pick_predictor(c_none: int, c_delta: int, c_zigzag: int):
    """The rule of predict="auto" on the three costs (any one unit) -> None, "delta" or "zigzag": the cheaper of the
    predictors that earn at least 1/64 of the cost without one, delta on a tie; None if neither does."""
    best = None
    for name, c in (("delta", int(c_delta)), ("zigzag", int(c_zigzag))):
        if 64 * c < 63 * int(c_none) and (best is None or c < best[1]):
            best = (name, c)
    return best[0] if best else None

CANDIDATES = (None, "delta", "zigzag", "xor", "sub", "subzz")  # by number: include/rcx_typed_stats.h, RCX_CAND_*
_CANDIDATE_ORDER = (1, 2, 5, 4, 3)  # ties: what needs no base first, subzz the default among the ops


def pick_candidate(costs, asked: int = 0x3F):
    """The rule of "auto" on the six costs of an item (any one unit; include/rcx_typed_stats.h) -> a name of CANDIDATES.
    asked: bit c = candidate c was measured.  A candidate other than none qualifies if 64 * C < 63 * C_none; the cheapest
    qualifying one wins, ties in the order delta, zigzag, subzz, sub, xor; None if nothing qualifies.  On the predictors alone
    it is pick_predictor."""
    if not asked & 1:
        raise ContainerError("the rule compares against the cost without a transform: candidate 0 must be asked for")
    best = None
    for c in _CANDIDATE_ORDER:
        if asked >> c & 1 and 64 * int(costs[c]) < 63 * int(costs[0]) and (best is None or int(costs[c]) < best[1]):
            best = (CANDIDATES[c], int(costs[c]))
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
    auto = _is_auto(predict)
    if not auto and (not (predict is None or isinstance(predict, str)) or predict not in PREDICTORS):
        raise ContainerError(f"a predictor is None, 'delta', 'zigzag' or 'auto', not {predict!r}")
    pred = 0 if auto else PREDICTORS[predict]  # (nothing to measure in an empty buffer: none, version 1)
    src, size = _source(data)
    width = _element_width(size, width, WIDTHS, "2, 4 or 8")
    import torch
    from . import predict as predictor, rcx
    n = _size(src)
    if n == 0:
        return typed_header_bytes(coder, block, 0, width, np.zeros(1, np.uint64), np.zeros(0, np.uint32) if checksum else None, pred)
    with _scope(ctx) as ctx:
        d_src = _on_device(src)
        d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
        held = None  # the predictor whose split text d_split holds
        if auto:
            choice, held = _measured_predictor(ctx, d_src, width, block, rcx.block_count(n, block), d_split)
            pred = PREDICTORS[choice]
        if held != pred:
            predictor.split_device(ctx, d_src, width, block, pred, d_split)  # (no predictor: the plane filter's own kernel)
        payload, offsets, crcs, raw = _encode_device(ctx, d_split, block, coder, checksum, gain)
        return typed_header_bytes(coder, block, n, width, offsets, crcs, pred, raw) + payload.tobytes()


def unpack_typed(blob, ctx=None, verify: bool = True) -> bytes:
    """Decode, verify the split text block by block if the container carries checksums (verify=False skips that), join."""
    import torch
    from . import predict as predictor
    c = parse_typed(blob)
    n = c["n"]
    if n == 0:
        return b""
    with _scope(ctx) as ctx:
        d_split = _decode_all_device(ctx, c, n, verify)
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        predictor.join_device(ctx, d_split, c["width"], c["block"], c["pred"], d_out)
        return d_out.cpu().numpy().tobytes()


def _cover(n: int, block: int, width: int, nblocks: int, start: int, stop: int):
    """The superblocks of width * block bytes that cover [start, stop) of n bytes -> (their blocks, where their span begins and
    ends in the data)."""
    superblock = width * block
    first, last = start // superblock, (stop - 1) // superblock
    return np.arange(first * width, min(nblocks, (last + 1) * width), dtype=np.uint64), first * superblock, min(n, (last + 1) * superblock)


def _decode_cover_device(ctx, c, pick, span: int, verify: bool):
    """The picked blocks follow one another and all but the container's last are whole: back to back they are the span's split text."""
    d_split, doffs = _decode_picked_device(ctx, c, block_lengths(c["n"], c["block"]), pick, "block", verify and c["crcs"] is not None)
    if int(doffs[-1]) != span:
        raise ContainerError("decoded size differs from the header")
    return d_split[:span]


def unpack_typed_range(blob, start: int, stop: int, ctx=None, verify: bool = True) -> bytes:
    """The bytes [start, stop) of the original: only the blocks of the superblocks that cover them are decoded and, in a
    container with checksums, verified; their span is joined as a buffer of its own."""
    import torch
    from . import predict as predictor
    c = parse_typed(blob)
    if not 0 <= start <= stop <= c["n"]:
        raise ContainerError("range outside the data")
    if start == stop:
        return b""
    pick, lo, hi = _cover(c["n"], c["block"], c["width"], c["nblocks"], start, stop)
    with _scope(ctx) as ctx:
        d_split = _decode_cover_device(ctx, c, pick, hi - lo, verify)
        d_out = torch.empty(hi - lo, dtype=torch.uint8, device="cuda")
        predictor.join_device(ctx, d_split, c["width"], c["block"], c["pred"], d_out)
        out = d_out.cpu().numpy()
    return out[start - lo: stop - lo].tobytes()


# ---- RCXD: residuals against a base in front of the plane filter -------------------------------------------------------------------
def _on_device(src):
    return src if hasattr(src, "numel") else _cuda(src)


def _verify_base_device(ctx, d_ref, block: int, crcs, first: int = 0) -> None:
    """d_ref: the base's bytes from its block `first` on, on the device; crcs: the table's entries for them."""
    ctx.verify_blocks_device(d_ref, block, _cuda(crcs))
    _raise_latched(ctx, lambda k: BaseMismatchError(first + k), "base block")


def pick_op(c_xor: int, c_sub: int, c_subzz: int) -> str:
    """The rule of pack_delta(op="auto") on the three costs: the cheapest, ties in the order subzz, sub, xor."""
    return min((int(c_subzz), 0, "subzz"), (int(c_sub), 1, "sub"), (int(c_xor), 2, "xor"))[2]


def _measured_op(ctx, d_src, d_ref, n: int, width: int, block: int) -> str:
    """pick_op on the sums over the superblocks: one measuring call with the superblocks as items against the base at the same
    offsets, three sums on the device, one download."""
    import torch
    from . import typed_stats
    count = -(-n // (width * block))
    offs = np.minimum(np.arange(count + 1, dtype=np.uint64) * np.uint64(width * block), np.uint64(n))
    d_cost = torch.zeros(typed_stats.CANDS * count, dtype=torch.int64, device="cuda")
    typed_stats.items_device(ctx, d_src, d_ref, offs, offs[:-1], np.full(count, width, np.uint8), np.full(count, typed_stats.OP_BITS, np.uint8), d_cost)
    sums = [int(v) for v in d_cost.view(count, typed_stats.CANDS).sum(dim=0).cpu()]  # (a superblock's cost is below 2^48)
    return pick_op(sums[typed_stats.XOR], sums[typed_stats.SUB], sums[typed_stats.SUBZZ])


def pack_delta(data, base, width=None, block: int = 65536, coder: int = 0, ctx=None, checksum: bool = False, stored=None, op: str = "subzz",
               base_check: bool = True) -> bytes:
    """data, base: each bytes, a numpy array or a contiguous torch tensor (CPU or GPU), of the same byte length -> an RCXD
    container of data's residual against base.  width=None: the element size of `data` (plain bytes need a width; 1, 2, 4 or
    8).  op: "xor", "sub" or "subzz" (include/rcx_base.h).  One upload each (none for GPU tensors), the residual and its planes in
    one kernel, then encode, mix and CRC-32 of the split text exactly as pack_typed does them; checksum= and stored= are the
    inner container's.  base_check: the CRC-32 of every block of the base goes into the prefix, the only guard against
    unpacking with another base.  op="auto": the cheapest of the three by the measured order-0 cost of the whole buffer
    (include/rcx_typed_stats.h on the superblock cut, the sums taken on the device, one download), ties in the order subzz, sub,
    xor, no margin; the container is byte for byte what that op given by name writes.  RCXD cannot say "no base": against an
    unrelated base every op loses to none, and only the item container (pack_delta_items, pack_tensors_delta) can decide that."""
    gain = _gain(stored)
    measured = _is_auto(op)
    if not measured and (not isinstance(op, str) or op not in BASE_OPS):
        raise ContainerError(f"an op is 'xor', 'sub', 'subzz' or 'auto', not {op!r}")
    op = "subzz" if measured else op  # (nothing to measure in an empty buffer)
    src, size = _source(data)
    ref = _source(base)[0]
    width = _element_width(size, width, ITEM_WIDTHS, "1, 2, 4 or 8")
    n = _size(src)
    if _size(ref) != n:
        raise ContainerError(f"the base has {_size(ref)} bytes, the data {n}: a base is as long as the data")

    def inner(offsets, crcs, raw):
        if width == 1:
            return header_bytes(coder, block, n, offsets, 0, crcs, raw)
        return typed_header_bytes(coder, block, n, width, offsets, crcs, 0, raw)

    if n == 0:
        none = np.zeros(0, np.uint32)
        return delta_header_bytes(BASE_OPS[op], width, block, 0, none if base_check else None) + inner(np.zeros(1, np.uint64), none if checksum else None, None)
    import torch
    from . import base as calls, rcx
    with _scope(ctx) as ctx:
        d_src, d_ref = _on_device(src), _on_device(ref)
        d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
        if measured:
            op = _measured_op(ctx, d_src, d_ref, n, width, block)
        calls.split_device(ctx, d_src, d_ref, width, block, BASE_OPS[op], d_split)
        if base_check:
            d_guard = torch.zeros(rcx.block_count(n, block), dtype=torch.int32, device="cuda")
            ctx.crc32_blocks_device(d_ref, block, d_guard)
        payload, offsets, crcs, raw = _encode_device(ctx, d_split, block, coder, checksum, gain)  # (one sync: the base's CRCs are there too)
        return delta_header_bytes(BASE_OPS[op], width, block, n, _crcs_of(d_guard) if base_check else None) + inner(offsets, crcs, raw) + payload.tobytes()


def _delta_base(c, base):
    ref = _source(base)[0]
    if _size(ref) != c["n"]:
        raise ContainerError(f"the base has {_size(ref)} bytes, the container was packed against one of {c['n']}")
    return ref


def unpack_delta(blob, base, ctx=None, verify: bool = True) -> bytes:
    """The base is verified against the prefix's table first (if it has one; verify=False skips that and the inner checksums),
    then decode as unpack_typed / unpack do, then the join against the base."""
    import torch
    from . import base as calls
    c = parse_delta(blob)
    ref = _delta_base(c, base)
    n = c["n"]
    if n == 0:
        return b""
    with _scope(ctx) as ctx:
        d_ref = _on_device(ref)
        if verify and c["base_crcs"] is not None:
            _verify_base_device(ctx, d_ref, c["block"], c["base_crcs"])
        d_split = _decode_all_device(ctx, c["inner"], n, verify)
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        calls.join_device(ctx, d_split, d_ref, c["width"], c["block"], c["op"], d_out)
        return d_out.cpu().numpy().tobytes()


def unpack_delta_range(blob, base, start: int, stop: int, ctx=None, verify: bool = True) -> bytes:
    """The bytes [start, stop) of the original: only the blocks of the superblocks that cover them are decoded (and, with
    inner checksums, verified), only those blocks of the base are verified, and the span is joined against the same span of
    the base as a buffer of its own."""
    import torch
    from . import base as calls
    c = parse_delta(blob)
    ref = _delta_base(c, base)
    block, width = c["block"], c["width"]
    if not 0 <= start <= stop <= c["n"]:
        raise ContainerError("range outside the data")
    if start == stop:
        return b""
    pick, lo, hi = _cover(c["n"], block, width, c["inner"]["nblocks"], start, stop)
    with _scope(ctx) as ctx:
        d_ref = _on_device(ref[lo:hi])
        if verify and c["base_crcs"] is not None:  # a superblock is whole blocks of the base: its blocks lo / block ..
            _verify_base_device(ctx, d_ref, block, c["base_crcs"][lo // block: lo // block + (hi - lo + block - 1) // block], lo // block)
        d_split = _decode_cover_device(ctx, c["inner"], pick, hi - lo, verify)
        d_out = torch.empty(hi - lo, dtype=torch.uint8, device="cuda")
        calls.join_device(ctx, d_split, d_ref, width, block, c["op"], d_out)
        out = d_out.cpu().numpy()
    return out[start - lo: stop - lo].tobytes()


# ---- RCXJ: a width and a predictor per buffer, in front of the item calls -----------------------------------------------------------
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
        if _is_auto(e):
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


def _pack_items_device(ctx, parts, lengths, widths, preds, auto, coder: int, checksum: bool, directory: bytes, gain, delta=None) -> bytes:
    """parts: the items that have bytes -> the container: one gather (an upload unless all lie on the device), split, encode over
    the sub-items, with a gain the mix of the stored sub-items behind it (the rule is applied to what was coded, after predict="auto"
    has decided), with checksum the CRC-32 of the sub-items of the split text, one download.  delta=None: RCXJ.  delta=(refs, ops,
    base_check): RCXK -- refs are the bases of those parts that have an op, gathered likewise; the one split call takes them, and
    one CRC call over the bases makes the guard."""
    lengths = np.asarray(lengths, dtype=np.uint64)
    _typed_items_tables(lengths, widths, preds)
    nsub, nitems = int(widths.astype(np.int64).sum()), len(widths)
    refs, ops, base_check = delta if delta is not None else (None, None, False)

    def blob(preds, offsets, crcs, raw, guard):
        prefix = b"" if delta is None else delta_items_header_bytes(ops, guard)
        return prefix + typed_items_header_bytes(coder, lengths, widths, preds, offsets, crcs, directory, raw)

    if int(lengths.sum()) == 0:  # nothing to code: no GPU
        crcs = np.zeros(nsub, np.uint32) if checksum else None
        return blob(preds, np.zeros(nsub + 1, np.uint64), crcs, None, np.zeros(nitems, np.uint32) if base_check else None)
    import torch
    from . import base_items, rcx, typed_items
    d_src = _gather_device(parts)
    d_ref = None if delta is None else _gather_device(refs)
    with _scope(ctx) as ctx:
        offs = rcx.item_offsets(lengths)
        sub_offs = typed_items.sub_offsets(offs, widths)
        d_split = torch.empty(d_src.numel(), dtype=torch.uint8, device="cuda")
        if auto.any():  # (only items without an op are measured; the others go through as planes there and are not looked at)
            preds = _measured_item_predictors(ctx, d_src, offs, widths, sub_offs, preds, auto, d_split)
        if delta is None:
            typed_items.split_device(ctx, d_src, offs, widths, preds, d_split)
        else:
            boffs = _base_offsets(lengths, ops)
            base_items.split_device(ctx, d_src, d_ref if d_ref.numel() else None, offs, boffs[:-1], widths, preds, ops, d_split)
        if base_check:
            d_guard = torch.zeros(nitems, dtype=torch.int32, device="cuda")
            if d_ref.numel():
                ctx.crc32_items_device(d_ref, boffs, d_guard)
        payload, offsets, crcs, raw = _encode_device(ctx, d_split, sub_offs, coder, checksum, gain)  # (one sync: the bases' CRCs are there too)
        guard = np.where((ops != BASE_OP_NONE) & (lengths > 0), _crcs_of(d_guard), 0).astype(np.uint32) if base_check else None
        return blob(preds, offsets, crcs, raw, guard) + payload.tobytes()


def pack_typed_items(items, widths=None, predict=None, coder: int = 0, ctx=None, checksum: bool = False, directory: bytes = b"", stored=None) -> bytes:
    """items: a list of buffers (bytes, numpy arrays, contiguous torch tensors on the CPU or the GPU) -> an RCXJ container.
    widths=None: each array's or tensor's element size (plain bytes need a width); else one width for all, or one per item.
    predict: None, "delta", "zigzag", "auto", or a list with one of these per item; "auto" decides per item from the measured
    order-0 costs (the module's docstring), and a width-1 item is never predicted.  One upload (none if every item lies on the
    GPU), then split, encode over the sub-items and, with checksum=True, their CRC-32, all with the device calls.
    stored=True | fraction: sub-items of the split text that do not shrink (by that fraction of their length) are kept raw and
    decoded by copy, so the payload never exceeds the items; the container is version 2 if there is such a sub-item, else the one
    written without the option.  With widths=1 that is the stored item container (pack_items has none)."""
    gain = _gain(stored)
    sources = [_source(x) for x in items]
    w = _item_widths(sources, widths)
    preds, auto = _item_predictors(predict, w)
    parts = [x for x, _ in sources]
    lengths = np.array([_size(x) for x in parts], dtype=np.uint64)
    return _pack_items_device(ctx, parts, lengths, w, preds, auto, coder, checksum, directory, gain)


def _sub_items(sub_first, widths, lengths, pick):
    """The picks' sub-items of an RCXJ container, in order: back to back they are the split text of the picks back to back
    -> (the sub-items, the pick that owns each, the picks' offsets back to back, their sub-items' offsets).  pick: int64, not empty."""
    from . import rcx, typed_items
    subs = np.concatenate([np.arange(sub_first[k], sub_first[k + 1], dtype=np.int64) for k in pick])
    doffs = rcx.item_offsets(lengths[pick])
    return subs, np.repeat(pick, widths[pick].astype(np.int64)), doffs, typed_items.sub_offsets(doffs, widths[pick])


def _unpack_items_device(ctx, c, pick, verify: bool, delta=None):
    """The picked items of a parsed RCXJ container, decoded, verified and joined on the device -> (the device buffer, the table of
    where each pick lies in it).  Only the picks' sub-items are decoded and checked.  delta=None: RCXJ.  delta=(k, refs, name): c
    is the inner container of the parsed RCXK container k and refs are the bases of the picks that have an op and bytes, in the
    picks' order: they are verified first, on the device, back to back (a pick without a base has length 0 there;
    BaseItemMismatchError carries name(item)), and the join is the one against the bases."""
    import torch
    from . import base_items, typed_items
    pick = np.asarray(pick, dtype=np.int64)
    widths, preds = c["widths"][pick], c["preds"][pick]
    subs, owner, doffs, soffs = _sub_items(c["sub_first"], c["widths"], c["lengths"], pick)
    n = int(doffs[-1])
    d_out = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    if n == 0:
        return d_out, doffs
    if delta is not None:
        k, refs, name = delta
        ops = k["ops"][pick]
        boffs = _base_offsets(c["lengths"][pick], ops)
        d_ref = _gather_device(refs)
        if int(boffs[-1]) != d_ref.numel():
            raise ContainerError("the bases are not as long as their items")
        if verify and k["base_crcs"] is not None and d_ref.numel():
            ctx.verify_items_device(d_ref, boffs, _cuda(k["base_crcs"][pick]))
            _raise_latched(ctx, lambda at: BaseItemMismatchError(int(pick[at]), name(int(pick[at]))), "the base of item")
    d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
    _decode_streams_device(ctx, c, soffs, d_split, subs.astype(np.uint64))  # (version 2: the stored sub-items are copied)
    if verify and c["crcs"] is not None:
        _verify_items_device(ctx, d_split, soffs, c["crcs"][subs], "item", owner)
    if delta is None:
        typed_items.join_device(ctx, d_split, doffs, widths, preds, d_out)
    else:
        base_items.join_device(ctx, d_split, d_ref if d_ref.numel() else None, doffs, boffs[:-1], widths, preds, ops, d_out)
    return d_out, doffs


def _picked(nitems: int, pick):
    if pick is not None and any(not 0 <= int(k) < nitems for k in pick):
        raise ContainerError("no such item")
    return np.arange(nitems, dtype=np.int64) if pick is None else np.array([int(k) for k in pick], dtype=np.int64)


def _unpack_picked(ctx, c, picked, verify: bool, delta=None) -> list:
    with _scope(ctx) as ctx:
        d_out, doffs = _unpack_items_device(ctx, c, picked, verify, delta)
        out = d_out.cpu().numpy()
        return [out[int(doffs[k]): int(doffs[k + 1])].tobytes() for k in range(len(picked))]


def unpack_typed_items(blob, pick=None, ctx=None, verify: bool = True) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None); picks may repeat or be empty.  Only the
    picked items' sub-items are decoded, and in a container with checksums only they are verified: a mismatch raises
    ChecksumError naming the item."""
    c = parse_typed_items(blob)
    picked = _picked(c["nitems"], pick)
    if len(picked) == 0:
        return []
    if int(c["lengths"][picked].sum()) == 0:
        return [b""] * len(picked)
    return _unpack_picked(ctx, c, picked, verify)


class OpenTypedItems(_Opened):
    """A typed item container on the device (open_typed_items): payload, stream table, stored flags, the items' lengths, widths
    and predictors and sub_first are uploaded once; decode_into enqueues the sub-items' decode into a staging buffer
    (include/rcx_picks.h) and their join to where the caller wants the items (include/rcx_typed_picks.h), picks, destinations
    and count read on the device.  Both calls' tables have SLOTS entries a pick, so that a latched position of either stage
    names the pick: pick_of."""

    SLOTS = 8  # table entries a pick: its sub-items in the decode call (a width is 8 at the most), itself in the first one of the join call

    def __init__(self, c, ctx):
        import torch
        from . import typed_picks
        self.nsub = c["nsub"]
        self.widths, self.preds = np.array(c["widths"], dtype=np.uint8), np.array(c["preds"], dtype=np.uint8)
        self.sub_first = np.array(c["sub_first"], dtype=np.int64)
        self.max_sub_len = int(c["sub_lengths"].max()) if self.nsub else 0
        super().__init__(c, c["lengths"], c["offsets"], c.get("stored"), c["crcs"], ctx)
        some = self.nitems > 0
        self.d_widths = _cuda(self.widths if some else np.ones(1, np.uint8)).to(torch.int64)
        self.d_preds = _cuda(self.preds if some else np.zeros(1, np.uint8)).to(torch.int64)
        self.d_sub_first = _cuda(self.sub_first)
        self.max_bytes, self.d_stage = 0, None
        self._join = typed_picks

    def reserve(self, max_pick: int, max_bytes: int) -> None:
        """The scratch of decode_into calls with at most max_pick picks of at most max_bytes together, and the staging buffer of
        max_bytes: after it they allocate nothing in the context."""
        import torch
        self._picks.reserve(self.ctx, self.SLOTS * max_pick, self.max_sub_len, self.coder)
        self._join.reserve(self.ctx, self.SLOTS * max_pick, max_bytes)
        self.max_bytes = int(max_bytes)
        self.d_stage = torch.zeros(max(self.max_bytes, 16), dtype=torch.uint8, device="cuda")

    def pick_of(self, position: int) -> int:
        """The pick position k that a latched position of decode_into names (sync_status()[1]), whichever stage latched it."""
        return int(position) // self.SLOTS

    def decode_into(self, d_pick, d_dst_at, d_count, d_dst, max_pick: int | None = None, stream=None) -> None:
        """Entry k < d_count[0]: item d_pick[k], joined -> d_dst[d_dst_at[k] : + its length].  d_pick, d_dst_at: int64 cuda tensors
        [>= max_pick]; d_count: an int64 cuda tensor of one entry; d_dst: a uint8 cuda tensor; reserve() comes first, and the picked
        items have at most its max_bytes between them (else nothing is joined and RCX_E_CAPACITY is latched).  Enqueues only, all of
        it on `stream` (a torch stream; None: the current one).  An entry that names no item is skipped and latched; entries at or past
        the count may hold anything.  Failures are the context's: sync_status(), its position through pick_of."""
        t = self._expand(d_pick, d_dst_at, d_count, max_pick, stream)
        self._picks.decode_device(self.ctx, self.d_payload, self.payload_size, self.d_offsets, t["sub_stream"], t["sub_at"], t["sub_len"], t["count"], self.d_stage,
                                  self.max_sub_len, max_pick=t["slots"], stored=self.d_stored, coder=self.coder, stream=stream, dst_cap=self.max_bytes)
        self._join.join_device(self.ctx, self.d_stage, t["from_at"], t["to_at"], t["item_len"], t["widths"], t["preds"], t["count"], d_dst,
                               self.max_bytes, max_pick=t["slots"], stream=stream, src_cap=self.max_bytes)

    def _expand(self, d_pick, d_dst_at, d_count, max_pick, stream, per_item=()):
        """The lookup of decode_into, by torch ops on `stream`: the picks' items, lengths and widths, and both calls' tables of
        SLOTS entries a pick -> dict.  per_item: (name, an int64 device table with an entry per item, what a pick that names no
        item and the slots behind the first get, the dtype) -> that table's entry of the pick in its first slot, under `name`."""
        import torch
        if self.d_stage is None:
            raise ContainerError("reserve(max_pick, max_bytes) comes first: it makes the staging buffer")
        max_pick = d_pick.numel() if max_pick is None else int(max_pick)
        S = self.SLOTS
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            p = d_pick[:max_pick]
            meant = torch.arange(max_pick, device=p.device) < d_count[:1]
            inside = meant & (p >= 0) & (p < self.nitems)
            item = torch.where(inside, p, torch.zeros_like(p))
            zero = torch.zeros_like(p)
            length = torch.where(inside, self.d_lengths[item], zero)
            w = torch.where(inside, self.d_widths[item], torch.ones_like(p))
            stage_at = torch.cumsum(length, 0) - length
            # the decode call's tables: slot q < w of pick k is its plane q, m bytes at q * m of the pick's staging span, the last with the tail
            q = torch.arange(S, device=p.device).unsqueeze(0)
            m = (length // w).unsqueeze(1)
            tail = (length - (length // w) * w).unsqueeze(1)
            live = q < w.unsqueeze(1)
            sub_len = torch.where(live, m + torch.where(q == w.unsqueeze(1) - 1, tail, torch.zeros_like(tail)), torch.zeros_like(q))
            sub_stream = self.d_sub_first[item].unsqueeze(1) + q
            sub_at = stage_at.unsqueeze(1) + q * m
            # a pick that names no item: a stream that does not exist, so that the call skips it and latches the pick
            lost = (meant & ~inside).unsqueeze(1) & (q == 0)
            sub_len = torch.where(lost, torch.ones_like(sub_len), sub_len)
            sub_stream = torch.where(lost, torch.full_like(sub_stream, self.nsub), sub_stream)
            count = d_count[:1] * S
            # the join call's tables: the pick itself in its first slot, the others empty
            first = (q == 0).to(torch.int64)
            from_at = (stage_at.unsqueeze(1) * first).contiguous()
            to_at = (torch.where(inside, d_dst_at[:max_pick], zero).unsqueeze(1) * first).contiguous()
            item_len = (length.unsqueeze(1) * first).contiguous()
            widths = (w.unsqueeze(1) * first + (1 - first)).to(torch.uint8).contiguous()
            preds = (torch.where(inside, self.d_preds[item], zero).unsqueeze(1) * first).to(torch.uint8).contiguous()
            out = {"slots": S * max_pick, "count": count, "sub_stream": sub_stream.contiguous().view(-1), "sub_at": sub_at.contiguous().view(-1),
                   "sub_len": sub_len.contiguous().view(-1), "from_at": from_at.view(-1), "to_at": to_at.view(-1), "item_len": item_len.view(-1),
                   "widths": widths.view(-1), "preds": preds.view(-1)}
            for name, table, missing, dtype in per_item:
                mine = torch.where(inside, table[item], torch.full_like(p, missing)).unsqueeze(1)
                out[name] = (mine * first + missing * (1 - first)).to(dtype).contiguous().view(-1)
            return out

    def verify(self, pick) -> None:
        """After decode_into whose picks were `pick` (a HOST table, all of them valid) and a synchronisation: the CRC-32 check of a
        container with checksums over the sub-items in the staging buffer, on the device -> ChecksumError naming the item."""
        if self.crcs is None:
            return
        pick = np.asarray(pick, dtype=np.int64)
        if len(pick) == 0 or int(self.lengths[pick].sum()) == 0:
            return
        subs, owner, _, soffs = _sub_items(self.sub_first, self.widths, self.lengths, pick)
        _verify_items_device(self.ctx, self.d_stage, soffs, self.crcs[subs], "item", owner)


def open_typed_items(blob, ctx=None) -> OpenTypedItems:
    """Any RCXJ container -- version 1 or 2, any widths and predictors, stored sub-items, with or without checksums -- parsed
    once and put on the device -> OpenTypedItems, whose decode_into takes picks, destinations and their count from device memory,
    decodes and joins, and can be captured in a graph.  ctx=None: a context of its own, closed by close()."""
    return OpenTypedItems(parse_typed_items(blob), ctx)


def __getattr__(name):
    """container.open_delta_items and container.OpenDeltaItems: the RCXK container opened on the device lives in delta_open.py
    (it builds on OpenTypedItems above) and is looked up there when it is asked for.  container.pack_items_device and
    container.PackedItems -- items that device code chose, encoded where they lie -- live in encode_picks.py in the same way, and
    container.pack_typed_items_device and container.PackedTypedItems -- typed items that device code chose, split and encoded where
    they lie -- in typed_split_picks.py."""
    if name in ("open_delta_items", "OpenDeltaItems"):
        from . import delta_open
        return getattr(delta_open, name)
    if name in ("pack_items_device", "PackedItems"):
        from . import encode_picks
        return getattr(encode_picks, name)
    if name in ("pack_typed_items_device", "PackedTypedItems"):
        from . import typed_split_picks
        return getattr(typed_split_picks, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---- tensors with names, on top of the typed item container ---------------------------------------------------------------
def _as_tensor(name, t):
    import torch
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t if t.flags.c_contiguous else np.ascontiguousarray(t))
    if type(t).__module__.split(".")[0] != "torch":
        raise ContainerError(f"{name!r} is neither a numpy array nor a torch tensor")
    return t


def _same_kind(a, b) -> bool:
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)


_Cut = collections.namedtuple("_Cut", "name tensor src width first lengths entry")  # a tensor as items: its bytes, its first item, the items' lengths, its entry


def _cut_tensors(named, block: int):
    """Every tensor of a state dict cut into typed items of element_size * block bytes, its superblocks, one after another -> _Cut.
    A generator: what a caller checks of one tensor is checked before the next tensor is looked at."""
    first = 0
    for name, t in named.items():
        t = _as_tensor(name, t)
        src, width = _source(t)
        if width not in ITEM_WIDTHS:
            raise ContainerError(f"{name!r}: an element is 1, 2, 4 or 8 bytes wide, not {width}")
        nbytes = _size(src)
        count = -(-nbytes // (width * block))
        lengths = [width * block] * (count - 1) + [nbytes - (count - 1) * width * block] if nbytes else []
        yield _Cut(name, t, src, width, first, lengths,
                   {"name": name, "dtype": str(t.dtype).replace("torch.", ""), "shape": tuple(t.shape), "first": first, "count": count})
        first += count


def _its_base(cut, base):
    """The base's tensor of that name, if it has the same dtype and shape; else None."""
    theirs = _as_tensor(cut.name, base[cut.name]) if cut.name in base else None
    return theirs if theirs is not None and _same_kind(theirs, cut.tensor) else None


def _of(option, name):
    return option.get(name) if isinstance(option, dict) else option


def _block_checked(block: int) -> None:
    if not 16 <= block <= MAX_ITEM:
        raise ContainerError("a block is 16 bytes to RCX_MAX_BLOCK")


def pack_tensors(named, block: int = 65536, predict=None, coder: int = 0, ctx=None, checksum: bool = False, stored=None) -> bytes:
    """named: a dict of names -> numpy arrays or contiguous torch tensors (CPU or GPU) -> an RCXJ container whose directory
    names them.  Every tensor is cut into typed items of element_size * block bytes, its superblocks.  predict: None, a
    name or "auto" for all tensors, or a dict of names -> those (a name it lacks: none); tensors of 1-byte elements are never
    predicted.  An element size outside 1, 2, 4, 8 raises ContainerError.  stored=True | fraction: as in pack_typed_items -- the
    sub-items are the blocks pack_typed(..., stored=...) would keep raw, the low mantissa planes of floating-point tensors."""
    gain = _gain(stored)
    _block_checked(block)
    parts, lengths, widths, entry_preds, entries = [], [], [], [], []
    for cut in _cut_tensors(named, block):
        entries.append(cut.entry)
        if cut.lengths:
            parts.append(cut.src)
            lengths += cut.lengths
            widths += [cut.width] * len(cut.lengths)
            entry_preds += [None if cut.width == 1 else _of(predict, cut.name)] * len(cut.lengths)
    w = np.array(widths, dtype=np.uint8)
    preds, auto = _item_predictors(entry_preds, w)
    return _pack_items_device(ctx, parts, np.array(lengths, dtype=np.uint64), w, preds, auto, coder, checksum, tensor_directory_bytes(entries), gain)


def _wanted(c, names):
    """The directory of a parsed RCXJ container and the tensors asked for -> (the names, their entries by name, their items)."""
    import torch
    entries = parse_tensor_directory(c["directory"], c["nitems"])
    by_name = {e["name"]: e for e in entries}
    wanted = [e["name"] for e in entries] if names is None else list(names)
    if any(n not in by_name for n in wanted):
        raise ContainerError("no such tensor")
    for n in wanted:
        if not isinstance(getattr(torch, by_name[n]["dtype"], None), torch.dtype):
            raise ContainerError(f"{by_name[n]['dtype']!r} is no torch dtype")
    pick = np.concatenate([np.arange(by_name[n]["first"], by_name[n]["first"] + by_name[n]["count"], dtype=np.int64) for n in wanted] + [np.zeros(0, np.int64)])
    return wanted, by_name, pick


def _unpack_tensors(ctx, c, wanted, by_name, pick, device: str, verify: bool, delta=lambda: None) -> dict:
    """The picked items of the parsed RCXJ container c, decoded if any has bytes (delta(): what _unpack_items_device takes, made
    only then), and the wanted tensors rebuilt from them, on `device`."""
    import torch
    from . import rcx
    out, at = {}, 0
    flat, doffs = None, rcx.item_offsets(c["lengths"][pick])
    if int(doffs[-1]):
        how = delta()
        with _scope(ctx) as ctx:
            flat, _ = _unpack_items_device(ctx, c, pick, verify, how)
            flat = flat if device == "cuda" else flat.cpu()
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


def unpack_tensors(blob, names=None, device: str = "cpu", ctx=None, verify: bool = True) -> dict:
    """-> a dict of torch tensors of the recorded dtype and shape, on `device` ("cuda": no download).  names: only those
    tensors, and only their items are decoded (and verified)."""
    c = parse_typed_items(blob)
    return _unpack_tensors(ctx, c, *_wanted(c, names), device, verify)


# ---- RCXK: an op against a base of its own, or a predictor, or neither, per buffer ----------------------------------------------
def _item_ops(ops, has_base):
    """ops: a name for every item that has a base, or one entry per item (a name, or None: no op) -> uint8[nitems]"""
    nitems = len(has_base)
    entries = list(ops) if isinstance(ops, (list, tuple)) else [ops if has_base[i] else None for i in range(nitems)]
    if len(entries) != nitems:
        raise ContainerError("one op per item")
    out = np.full(nitems, BASE_OP_NONE, np.uint8)
    for i, e in enumerate(entries):
        if e is None:
            continue
        if not isinstance(e, str) or e not in BASE_OPS:
            raise ContainerError(f"an op is 'xor', 'sub', 'subzz' or None, not {e!r}")
        if not has_base[i]:
            raise ContainerError(f"item {i} has an op and no base")
        out[i] = BASE_OPS[e]
    return out


def _base_offsets(lengths, ops):
    """The bases of the items with an op back to back -> (their table of nitems + 1 offsets, where an item without one has length 0)"""
    from . import rcx
    return rcx.item_offsets(np.where(ops != BASE_OP_NONE, lengths, 0).astype(np.uint64))


def _item_widths(sources, widths):
    """widths=None: each source's element size; else one width for all, or one per item -> uint8[nitems], checked."""
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
    return np.array(each, dtype=np.uint8)


def _delta_item_predictors(predict, widths, ops):
    """predict applies to the items without an op; an explicit predictor on an item with one is refused."""
    based = ops != BASE_OP_NONE
    if isinstance(predict, (list, tuple)):
        if len(predict) != len(widths):
            raise ContainerError("one predictor per item")
        if any(e is not None for e, b in zip(predict, based) if b):
            raise ContainerError("an item with a base takes no predictor")
        return _item_predictors(list(predict), widths)
    return _item_predictors([None if b or w == 1 else predict for b, w in zip(based, widths)], widths)


def _is_auto(e) -> bool:
    return isinstance(e, str) and e == AUTO


def _says_auto(ops) -> bool:
    return _is_auto(ops) or (isinstance(ops, (list, tuple)) and any(_is_auto(e) for e in ops)) or (isinstance(ops, dict) and any(_is_auto(e) for e in ops.values()))


def _delta_item_masks(ops, predict, has_base, widths):
    """ops, predict as pack_delta_items takes them, "auto" among them -> (masks uint8[nitems]: the candidates to measure per item,
    bit c = candidate c of CANDIDATES, 0 for an item that is named; the op and the predictor entry per item, None where the
    measurement decides).  An "auto" op needs a base; such an item's predictor entry is None (none and the three ops are
    measured) or "auto" (all six, at width above 1); a named one raises in the list form and is not applied in the scalar form."""
    nitems = len(widths)
    each_op, each_pred = isinstance(ops, (list, tuple)), isinstance(predict, (list, tuple))
    op_entries = list(ops) if each_op else [ops if has_base[i] else None for i in range(nitems)]
    pred_entries = list(predict) if each_pred else [predict] * nitems
    if len(op_entries) != nitems:
        raise ContainerError("one op per item")
    if len(pred_entries) != nitems:
        raise ContainerError("one predictor per item")
    masks = np.zeros(nitems, np.uint8)
    for i, (o, p) in enumerate(zip(op_entries, pred_entries)):
        if not (o is None or _is_auto(o) or (isinstance(o, str) and o in BASE_OPS)):
            raise ContainerError(f"an op is 'xor', 'sub', 'subzz', 'auto' or None, not {o!r}")
        if not (p is None or _is_auto(p) or (isinstance(p, str) and p in PREDICTORS)):
            raise ContainerError(f"a predictor is None, 'delta', 'zigzag' or 'auto', not {p!r}")
        if o is not None and not has_base[i]:
            raise ContainerError(f"item {i} has an op and no base")
        if _is_auto(o):
            if p is not None and not _is_auto(p) and each_pred:
                raise ContainerError("an item with a base takes no predictor")
            masks[i] = 0x3F if _is_auto(p) and widths[i] > 1 else 0x39
            op_entries[i] = pred_entries[i] = None
        elif o is None:
            if _is_auto(p):
                masks[i] = 0x07 if widths[i] > 1 else 0
                pred_entries[i] = None
            elif not each_pred and widths[i] == 1:
                pred_entries[i] = None
        elif not each_pred:
            pred_entries[i] = None  # (a named op: the scalar predictor is for the items without one)
    return masks, op_entries, pred_entries


def _no_costs(nitems: int) -> np.ndarray:
    """Nothing to measure: every cost is 0, and the rule says none."""
    return np.zeros((nitems, len(CANDIDATES)), np.uint64)


def _decided(costs, masks, op_entries, pred_entries, groups=None):
    """pick_candidate per measured item -- per group of items (first, count) on the sums over the group, if groups are given: a
    tensor takes its base entirely or not at all -> (ops, predict): a name or None per item."""
    costs = np.asarray(costs, dtype=np.uint64).reshape(len(masks), len(CANDIDATES))
    ops, preds = list(op_entries), list(pred_entries)
    for first, count in (groups if groups is not None else [(i, 1) for i in range(len(masks))]):
        if count == 0 or not masks[first]:
            continue
        sums = [sum(int(v) for v in costs[first: first + count, c]) for c in range(len(CANDIDATES))]
        choice = pick_candidate(sums, int(masks[first]))
        for i in range(first, first + count):
            ops[i] = choice if choice in BASE_OPS else None
            preds[i] = choice if choice is not None and choice not in BASE_OPS else None
    return ops, preds


def _need(masks, lengths):
    """The items whose base a measurement reads: their mask has an op bit and they have bytes."""
    from . import typed_stats
    return ((masks & typed_stats.OP_BITS) != 0) & (lengths > 0)


def _measured_costs(ctx, live, needed, lengths, widths, masks):
    """live: the buffers that have bytes, back to back the items in order; needed: likewise the bases of the items of _need
    -> (costs uint64[nitems, 6], the two device buffers, the items' offsets in them).  One measuring call for everything a pack has
    to measure (include/rcx_typed_stats.h); one gather (an upload unless all lie on the device) each for the items and the bases."""
    import torch
    from . import rcx, typed_stats
    nitems = len(widths)
    d_src, d_ref = _gather_device(live), _gather_device(needed)
    offs, boffs = rcx.item_offsets(lengths), rcx.item_offsets(np.where(_need(masks, lengths), lengths, 0).astype(np.uint64))
    d_cost = torch.zeros(typed_stats.CANDS * nitems, dtype=torch.int64, device="cuda")
    if masks.any():
        typed_stats.items_device(ctx, d_src, d_ref if d_ref.numel() else None, offs, boffs[:-1], widths, masks, d_cost)
    return d_cost.cpu().numpy().view(np.uint64).reshape(nitems, typed_stats.CANDS), d_src, d_ref, offs, boffs


def _measured_candidates(ctx, parts, theirs, lengths, widths, masks):
    """_measured_costs on items and their bases -> (costs; the items as views of the one device buffer; the bases likewise, those
    the measurement did not need as they were)."""
    need = _need(masks, lengths)
    costs, d_src, d_ref, offs, boffs = _measured_costs(ctx, [x for x in parts if _size(x)], [theirs[i] for i in np.flatnonzero(need)], lengths, widths, masks)
    views = [d_src[int(offs[i]): int(offs[i + 1])] for i in range(len(widths))]
    bases = [d_ref[int(boffs[i]): int(boffs[i + 1])] if need[i] else theirs[i] for i in range(len(widths))]
    return costs, views, bases


def _delta_items_inputs(items, bases, widths):
    """-> (the items' bytes, their bases' bytes or None, lengths uint64[nitems], widths uint8[nitems]), checked."""
    sources = [_source(x) for x in items]
    if len(bases) != len(sources):
        raise ContainerError("one base, or None, per item")
    w = _item_widths(sources, widths)
    parts = [x for x, _ in sources]
    lengths = np.array([_size(x) for x in parts], dtype=np.uint64)
    theirs = [None if b is None else _source(b)[0] for b in bases]
    for i, b in enumerate(theirs):
        if b is not None and _size(b) != int(lengths[i]):
            raise ContainerError(f"the base of item {i} has {_size(b)} bytes, the item {int(lengths[i])}: a base is as long as its item")
    return parts, theirs, lengths, w


def choose_delta_items_from_costs(costs, has_base, widths, ops="auto", predict=None):
    """The decision of choose_delta_items from a table of costs [nitems, 6] (typed_stats.costs_numpy or the device call), without
    a GPU: has_base and widths per item, ops and predict as pack_delta_items takes them -> (ops, predict), a name or None per
    item.  Only the entries the masks ask for are looked at (an "auto" op: none and the three ops, with predict "auto" all six; a
    predict "auto" without an op: none, delta, zigzag)."""
    w = np.asarray(widths, dtype=np.uint8)
    masks, op_entries, pred_entries = _delta_item_masks(ops, predict, list(has_base), w)
    return _decided(costs, masks, op_entries, pred_entries)


def delta_item_masks(has_base, widths, ops="auto", predict=None) -> np.ndarray:
    """The masks of include/rcx_typed_stats.h that pack_delta_items and choose_delta_items measure with, uint8[nitems]."""
    return _delta_item_masks(ops, predict, list(has_base), np.asarray(widths, dtype=np.uint8))[0]


def choose_delta_items(items, bases, widths=None, ops="auto", predict=None, ctx=None):
    """The decision pack_delta_items(..., ops=ops, predict=predict) makes, alone -> (ops, predict): lists with a name or None per
    item, which given back to pack_delta_items write the same container -- and tell which tensors lean on their base.  One
    measuring call on the GPU (include/rcx_typed_stats.h), the rule is pick_candidate."""
    parts, theirs, lengths, w = _delta_items_inputs(items, bases, widths)
    masks, op_entries, pred_entries = _delta_item_masks(ops, predict, [b is not None for b in theirs], w)
    if not masks.any() or not int(lengths.sum()):  # nothing to measure
        return _decided(_no_costs(len(w)), masks, op_entries, pred_entries)
    with _scope(ctx) as ctx:
        costs, _, _ = _measured_candidates(ctx, parts, theirs, lengths, w, masks)
    return _decided(costs, masks, op_entries, pred_entries)


def pack_delta_items(items, bases, widths=None, ops="subzz", predict=None, coder: int = 0, ctx=None, checksum: bool = False, directory: bytes = b"",
                     stored=None, base_check: bool = True) -> bytes:
    """items: a list of buffers as pack_typed_items takes them; bases: one entry per item, None or a buffer of the item's byte
    length (any other length raises ContainerError) -> an RCXK container.  ops: "xor", "sub" or "subzz" for every item that has
    a base, or a list with one of these or None per item (None: the item is packed without its base; an op on an item whose base
    is None raises).  predict: as in pack_typed_items, for the items without an op; an explicit predictor on an item with one
    raises.  One gather and upload for the items and one for the bases (none for what lies on the GPU), one split call, one encode
    over the sub-items, one CRC call for the guard, one download.  base_check: the CRC-32 of every item's base goes into the
    prefix, the only guard against unpacking with another base.
    "auto" as an entry of the list: the op of that item is measured (the module's docstring, pick_candidate; the one name
    ops="auto" for all stays refused here, as it always was: choose_delta_items takes it and returns the lists) -- one
    measuring call for everything the pack has to measure, the predict="auto" items without a base in it -- and may come out as
    no base at all; such an item's predict entry is None, or "auto" to put the predictors into the comparison.  Then the path
    is the one of the named choices, and the container byte for byte what choose_delta_items' lists given here write."""
    gain = _gain(stored)
    parts, theirs, lengths, w = _delta_items_inputs(items, bases, widths)

    def named(ctx, ops, predict, parts, theirs):
        o = _item_ops(ops, [b is not None for b in theirs])
        preds, auto = _delta_item_predictors(predict, w, o)
        refs = [b for b, op in zip(theirs, o) if op != BASE_OP_NONE and _size(b)]
        return _pack_items_device(ctx, [x for x in parts if _size(x)], lengths, w, preds, auto, coder, checksum, directory, gain, (refs, o, base_check))

    if not (isinstance(ops, (list, tuple)) and _says_auto(ops)):
        return named(ctx, ops, predict, parts, theirs)
    masks, op_entries, pred_entries = _delta_item_masks(ops, predict, [b is not None for b in theirs], w)
    if not int(lengths.sum()):  # nothing to measure
        return named(ctx, *_decided(_no_costs(len(w)), masks, op_entries, pred_entries), parts, theirs)
    with _scope(ctx) as ctx:
        costs, parts, theirs = _measured_candidates(ctx, parts, theirs, lengths, w, masks)
        return named(ctx, *_decided(costs, masks, op_entries, pred_entries), parts, theirs)


def _picked_bases(c, picked, base_of, what=lambda k: f"item {k}"):
    """The bases of the picks that have an op and bytes, each as long as its item; a missing one raises."""
    refs = []
    for k in picked:
        k = int(k)
        if c["ops"][k] == BASE_OP_NONE or int(c["inner"]["lengths"][k]) == 0:
            continue
        b = base_of(k)
        if b is None:
            raise ContainerError(f"{what(k)} was packed against a base, and there is none")
        b = _source(b)[0]
        if _size(b) != int(c["inner"]["lengths"][k]):
            raise ContainerError(f"the base of {what(k)} has {_size(b)} bytes, the item {int(c['inner']['lengths'][k])}")
        refs.append(b)
    return refs


def unpack_delta_items(blob, bases, pick=None, ctx=None, verify: bool = True) -> list:
    """-> the list of the picked items' bytes (all of them, in order, if pick is None).  bases: one entry per item of the
    container; only those of the picked items that have an op are looked at, the others may be None.  A missing base raises
    ContainerError.  The picked items' bases are verified against the prefix's table first (BaseItemMismatchError names the
    item), then only their sub-items are decoded and verified; verify=False skips the guard and the inner checksums."""
    c = parse_delta_items(blob)
    if len(bases) != c["nitems"]:
        raise ContainerError("one base, or None, per item of the container")
    picked = _picked(c["nitems"], pick)
    if len(picked) == 0:
        return []
    if int(c["inner"]["lengths"][picked].sum()) == 0:
        return [b""] * len(picked)
    refs = _picked_bases(c, picked, lambda k: bases[k])
    return _unpack_picked(ctx, c["inner"], picked, verify, (c, refs, lambda k: None))


_Row = collections.namedtuple("_Row", "name src ref first count op pred mask")  # a tensor of pack_tensors_delta: op, pred: None where measured


def _tensor_candidates(named, base, block: int, op, predict):
    """The items pack_tensors_delta cuts a state dict into, and what is to be measured of them -> dict(rows: a _Row per tensor;
    lengths, widths, masks per item)."""
    rows, lengths, widths, masks = [], [], [], []
    for cut in _cut_tensors(named, block):
        theirs = _its_base(cut, base)
        each_op = _of(op, cut.name) if theirs is not None else None
        m, o, p = _delta_item_masks([each_op], _of(predict, cut.name), [theirs is not None], np.array([cut.width], np.uint8))
        rows.append(_Row(cut.name, cut.src, None if theirs is None else _source(theirs)[0], cut.first, len(cut.lengths), o[0], p[0], int(m[0])))
        lengths += cut.lengths
        widths += [cut.width] * len(cut.lengths)
        masks += [int(m[0])] * len(cut.lengths)
    return {"rows": rows, "lengths": np.array(lengths, np.uint64), "widths": np.array(widths, np.uint8), "masks": np.array(masks, np.uint8)}


def tensor_delta_masks(named, base, block: int = 65536, op="auto", predict=None) -> dict:
    """What choose_tensors_delta measures, without a GPU -> dict(lengths, widths, masks per item; first: name -> (its first item,
    its item count)): the tables typed_stats.costs_numpy takes for choose_tensors_delta_from_costs."""
    c = _tensor_candidates(named, base, block, op, predict)
    return {"lengths": c["lengths"], "widths": c["widths"], "masks": c["masks"], "first": {r.name: (r.first, r.count) for r in c["rows"]}}


def _tensors_decided(c, costs=None):
    """costs=None: nothing was measured."""
    rows = c["rows"]
    costs = _no_costs(len(c["masks"])) if costs is None else costs
    ops, preds = _decided(costs, c["masks"], [r.op for r in rows for _ in range(r.count)], [r.pred for r in rows for _ in range(r.count)],
                          groups=[(r.first, r.count) for r in rows])
    # (a tensor without bytes has no item to ask: the rule on costs of 0 says none)
    return ({r.name: (ops[r.first] if r.count else None if r.mask else r.op) for r in rows},
            {r.name: (preds[r.first] if r.count else None if r.mask else r.pred) for r in rows})


def choose_tensors_delta_from_costs(costs, named, base, block: int = 65536, op="auto", predict=None):
    """The decision of choose_tensors_delta from a table of costs [nitems, 6] over the items of tensor_delta_masks, without a GPU."""
    return _tensors_decided(_tensor_candidates(named, base, block, op, predict), costs)


def choose_tensors_delta(named, base, block: int = 65536, op="auto", predict=None, ctx=None):
    """The decision pack_tensors_delta(..., op=op, predict=predict) makes, alone -> (op, predict): dicts of names -> a name or
    None, which given back to pack_tensors_delta write the same container.  Per TENSOR, pick_candidate on the sums over the
    tensor's items: a tensor needs its base entirely or not at all."""
    c = _tensor_candidates(named, base, block, op, predict)
    if not c["masks"].any():
        return _tensors_decided(c)
    from . import typed_stats
    with _scope(ctx) as ctx:
        live = [r.src for r in c["rows"] if r.count]
        needed = [r.ref for r in c["rows"] if r.count and r.mask & typed_stats.OP_BITS]
        return _tensors_decided(c, _measured_costs(ctx, live, needed, c["lengths"], c["widths"], c["masks"])[0])


def pack_tensors_delta(named, base, block: int = 65536, op="subzz", predict=None, coder: int = 0, ctx=None, checksum: bool = False, stored=None,
                       base_check: bool = True) -> bytes:
    """named, base: dicts of names -> numpy arrays or contiguous torch tensors (CPU or GPU) -> an RCXK container whose directory
    names the tensors of `named`: a state dict against the one before it.  A tensor gets the op if `base` holds its name with
    the same dtype and shape; every other tensor is packed as pack_tensors packs it, and `predict` (as in pack_tensors) applies
    to those only.  op: a name for all, or a dict of names -> a name or None (None, or a name it lacks: packed without its base);
    a name in the dict whose base is missing or of another dtype or shape raises ContainerError.  Every tensor is cut into
    items of element_size * block bytes, and its base with it."""
    gain = _gain(stored)
    _block_checked(block)
    if isinstance(op, dict):
        for name, e in op.items():
            if e is not None and name in named and not (name in base and _same_kind(_as_tensor(name, base[name]), _as_tensor(name, named[name]))):
                raise ContainerError(f"{name!r} has an op, and the base has no tensor of that name, dtype and shape")
    if _says_auto(op):
        c = _tensor_candidates(named, base, block, op, predict)
        if not c["masks"].any():
            return pack_tensors_delta(named, base, block, *_tensors_decided(c), coder, ctx, checksum, stored, base_check)
        with _scope(ctx) as ctx:  # what is measured and then packed goes up once
            named = {name: _as_tensor(name, t).cuda() for name, t in named.items()}
            base = {name: _as_tensor(name, base[name]).cuda() for name in named if name in base}
            op, predict = choose_tensors_delta(named, base, block, op, predict, ctx)
            return pack_tensors_delta(named, base, block, op, predict, coder, ctx, checksum, stored, base_check)
    parts, refs, lengths, widths, entry_preds, entry_ops, entries = [], [], [], [], [], [], []
    for cut in _cut_tensors(named, block):
        entries.append(cut.entry)
        theirs = _its_base(cut, base)
        each_op = _of(op, cut.name) if theirs is not None else None
        if cut.lengths:
            parts.append(cut.src)
            if each_op is not None:
                refs.append(_source(theirs)[0])
            lengths += cut.lengths
            widths += [cut.width] * len(cut.lengths)
            entry_preds += [None if cut.width == 1 or each_op is not None else _of(predict, cut.name)] * len(cut.lengths)
            entry_ops += [each_op] * len(cut.lengths)
    w = np.array(widths, dtype=np.uint8)
    o = _item_ops(entry_ops, [e is not None for e in entry_ops])
    preds, auto = _item_predictors(entry_preds, w)
    return _pack_items_device(ctx, parts, np.array(lengths, dtype=np.uint64), w, preds, auto, coder, checksum, tensor_directory_bytes(entries), gain,
                              (refs, o, base_check))


def unpack_tensors_delta(blob, base, names=None, device: str = "cpu", ctx=None, verify: bool = True) -> dict:
    """-> a dict of torch tensors of the recorded dtype and shape, on `device` ("cuda": no download).  names: only those
    tensors; only their items are decoded (and verified), and only their bases are needed and verified: a tensor that was
    packed against a base and is missing from `base`, or has another size there, raises ContainerError, one whose bytes differ
    BaseItemMismatchError with the item and the tensor's name."""
    c = parse_delta_items(blob)
    inner = c["inner"]
    wanted, by_name, pick = _wanted(inner, names)
    owner = {int(k): e["name"] for e in by_name.values() for k in range(e["first"], e["first"] + e["count"])}
    # the bases of the wanted tensors, cut as the tensors were: item k of a tensor is the same bytes of its base
    cut = {}
    for n in wanted:
        e = by_name[n]
        items = range(e["first"], e["first"] + e["count"])
        if not any(c["ops"][k] != BASE_OP_NONE and int(inner["lengths"][k]) for k in items):
            continue
        if n not in base:
            raise ContainerError(f"tensor {n!r} was packed against a base, and the base has none of that name")
        ref = _source(_as_tensor(n, base[n]))[0]
        if _size(ref) != int(inner["lengths"][e["first"]: e["first"] + e["count"]].sum()):
            raise ContainerError(f"tensor {n!r}: the base has {_size(ref)} bytes, not the tensor's")
        at = 0
        for k in items:
            cut[k] = ref[at: at + int(inner["lengths"][k])]
            at += int(inner["lengths"][k])
    return _unpack_tensors(ctx, inner, wanted, by_name, pick, device, verify,
                           lambda: (c, _picked_bases(c, pick, cut.get, lambda k: f"item {k} of tensor {owner.get(k)!r}"), owner.get))
