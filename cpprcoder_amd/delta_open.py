"""open_delta_items: an RCXK container (container.pack_delta_items) opened once on the device with its bases, for a reader that
picks on the GPU.  It is container.OpenTypedItems for the inner container, with the join against the bases
(include/rcx_base_picks.h, cpprcoder_amd/base_picks.py) behind the decode (include/rcx_picks.h).

The module is apart from container.py because that module's surface is pinned (tests/golden/container_parity.json records its
public names for the commits that only rearrange it); container.open_delta_items and container.OpenDeltaItems resolve to the
two names here when they are asked for (container.__getattr__), so a caller writes container.open_delta_items(blob, bases).
"""
from __future__ import annotations

import numpy as np

from .container import OpenTypedItems, _cuda, _gather_device, _raise_latched, _size, _source
from .layout import BASE_OP_NONE, BaseItemMismatchError, ContainerError, parse_delta_items


class OpenDeltaItems(OpenTypedItems):
    """A delta item container on the device (open_delta_items): what OpenTypedItems holds of the inner container, the items'
    ops, and the bases gathered into one device buffer with a base offset per item.  decode_into enqueues the sub-items' decode
    into the staging buffer (include/rcx_picks.h) and their join against the bases to where the caller wants the items
    (include/rcx_base_picks.h); reserve, pick_of and verify have OpenTypedItems' contract."""

    def __init__(self, k, bases, ctx, verify: bool = True):
        import torch
        from . import base_picks
        if len(bases) != k["nitems"]:
            raise ContainerError("one base, or None, per item of the container")
        super().__init__(k["inner"], ctx)
        self._join = base_picks
        self.ops = np.array(k["ops"], dtype=np.uint8)
        # the spans: entries that are the same object share one, in the order of their first item
        spans, parts, first_of, missing, at = {}, [], [], [], 0
        base_at = np.zeros(max(self.nitems, 1), dtype=np.uint64)
        for i in range(self.nitems):
            if self.ops[i] == BASE_OP_NONE or int(self.lengths[i]) == 0:
                continue
            if bases[i] is None:
                missing.append(i)
                continue
            if id(bases[i]) not in spans:
                src = _source(bases[i])[0]
                spans[id(bases[i])] = (at, _size(src), len(parts))
                parts.append(src)
                first_of.append(i)
                at += _size(src)
            where, size, _ = spans[id(bases[i])]
            if size != int(self.lengths[i]):
                raise ContainerError(f"the base of item {i} has {size} bytes, the item {int(self.lengths[i])}")
            base_at[i] = where
        self.base_cap = at
        base_at[missing] = at + 1  # past base_cap: a pick of such an item is skipped and latched RCX_E_CAPACITY
        self.d_base = _gather_device(parts) if at else torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.d_base_at = _cuda(base_at)
        self.d_ops = _cuda(self.ops if self.nitems else np.full(1, BASE_OP_NONE, np.uint8)).to(torch.int64)
        try:
            if verify and k["base_crcs"] is not None and at:
                from . import rcx
                crcs = np.array(k["base_crcs"], dtype=np.uint32)
                self.ctx.verify_items_device(self.d_base, rcx.item_offsets(np.array([_size(x) for x in parts], dtype=np.uint64)), _cuda(crcs[first_of]))
                _raise_latched(self.ctx, lambda span: BaseItemMismatchError(first_of[span]), "the base of item")
                for i in range(self.nitems):  # (the items that share a span: the same bytes have one CRC-32)
                    if self.ops[i] != BASE_OP_NONE and int(self.lengths[i]) and bases[i] is not None and crcs[i] != crcs[first_of[spans[id(bases[i])][2]]]:
                        raise BaseItemMismatchError(i)
        except Exception:
            self.close()
            raise

    def decode_into(self, d_pick, d_dst_at, d_count, d_dst, max_pick: int | None = None, stream=None) -> None:
        """OpenTypedItems.decode_into's contract (reserve comes first: it reserves for this join); an item with an op is joined against its base.  A pick of an item whose op needs a
        base that was given as None is skipped and latched RCX_E_CAPACITY at its pick; d_dst lies apart from the bases."""
        import torch
        t = self._expand(d_pick, d_dst_at, d_count, max_pick, stream, (("ops", self.d_ops, BASE_OP_NONE, torch.uint8), ("base_at", self.d_base_at, 0, torch.int64)))
        self._picks.decode_device(self.ctx, self.d_payload, self.payload_size, self.d_offsets, t["sub_stream"], t["sub_at"], t["sub_len"], t["count"], self.d_stage,
                                  self.max_sub_len, max_pick=t["slots"], stored=self.d_stored, coder=self.coder, stream=stream, dst_cap=self.max_bytes)
        self._join.join_device(self.ctx, self.d_stage, self.d_base, t["from_at"], t["base_at"], t["to_at"], t["item_len"], t["widths"], t["preds"], t["ops"],
                               t["count"], d_dst, self.max_bytes, max_pick=t["slots"], stream=stream, src_cap=self.max_bytes, base_cap=self.base_cap)


def open_delta_items(blob, bases, ctx=None, verify: bool = True) -> OpenDeltaItems:
    """Any RCXK container, parsed once and put on the device with its bases -> OpenDeltaItems, whose decode_into takes picks,
    destinations and their count from device memory, decodes, joins against the bases, and can be captured in a graph.  bases: one
    entry per item, or None; bytes-like objects and tensors, CUDA tensors as they are (not downloaded); entries that are the SAME
    OBJECT share one span of the device buffer -- one reference page for a thousand pages.  The CRC-32 guard of the prefix is
    checked once, here, on the GPU, for every item that has an op, bytes and a base: BaseItemMismatchError names the item;
    verify=False skips it.  ctx=None: a context of its own, closed by close()."""
    return OpenDeltaItems(parse_delta_items(blob), bases, ctx, verify)
