"""What tests/golden/container_parity.json records of the container layer (cpprcoder_amd/container.py and layout.py), and
how: tests/golden/make_golden_containers.py runs these functions at one commit and writes what they return, and
tests/test_container_parity_cpu.py and tests/test_gpu_container_parity.py run them again and compare.  Only public names of
`container` are used, so the same text runs on any commit that has them.

cpu_section(): no library, no GPU -- header bytes for argument sets that reach every branch of the four writers, every
refusal of the writers, the four parsers on valid blobs damaged byte by byte and cut at every length, and the calls that
return without a GPU.  gpu_cases(): name -> a function of (a recorder, a context) that packs, unpacks and checks the round
trip; the recorder keeps the blob's hash and length and, per public call, the ordered names of the rcx.Context methods and
of the module device calls it made.
"""
import contextlib
import hashlib
import types

import numpy as np

from cpprcoder_amd import container

CONSTANTS = ("MAGIC", "VERSION", "VERSION_CRC", "VERSION_STORED", "FLAG_BLKSORT", "FLAG_CRC32", "FLAG_STORED", "ITEM_MAGIC", "ITEM_VERSION", "MAX_ITEM",
             "TYPED_MAGIC", "TYPED_VERSION", "TYPED_VERSION_PRED", "TYPED_VERSION_STORED", "AUTO", "WIDTHS", "TYPED_ITEMS_MAGIC", "TYPED_ITEMS_VERSION", "ITEM_WIDTHS")
FIXED = {"RCXB": 28, "RCXI": 16, "RCXT": 36, "RCXJ": 32}  # bytes of each layout's fixed part
PARSERS = {"RCXB": "parse", "RCXI": "parse_items", "RCXT": "parse_typed", "RCXJ": "parse_typed_items"}


# ---- results as JSON ---------------------------------------------------------------------------------------------------------
def plain(v):
    """A parser's or a call's result as JSON: arrays as lists, bytes as hex."""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tobytes().hex() if v.dtype == np.uint8 and v.ndim == 1 and len(v) > 16 else [plain(x) for x in v.tolist()]
    if isinstance(v, (bytes, bytearray, memoryview)):
        return bytes(v).hex()
    if isinstance(v, (np.integer, np.bool_)):
        return v.item()
    if type(v).__module__.split(".")[0] == "torch":
        return {"dtype": str(v.dtype), "shape": list(v.shape), "device": v.device.type, "bytes": v.detach().cpu().contiguous().numpy().tobytes().hex()}
    return v


def outcome(fn, *args, **kwargs):
    """-> {"ok": the result} or {"error": the exception's class, "text": str(e)}"""
    try:
        return {"ok": plain(fn(*args, **kwargs))}
    except Exception as e:  # noqa: BLE001 (the class is what is recorded)
        return {"error": type(e).__name__, "text": str(e)}


def verdict(parser, blob) -> str:
    try:
        parser(blob)
        return "parsed"
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"


# ---- the CPU section ---------------------------------------------------------------------------------------------------------
def _payload(n: int, salt: int) -> bytes:
    return bytes((7 * i + salt) & 0xFF for i in range(n))


def header_sets():
    """name -> (writer, args, kwargs): every branch of the four writers, refusals included."""
    c = container
    big = c.MAX_ITEM + 1
    return {
        # RCXB
        "RCXB plain": ("header_bytes", (0, 16, 40, [0, 5, 12, 20]), {}),
        "RCXB blksort": ("header_bytes", (1, 16, 40, [0, 5, 12, 20], c.FLAG_BLKSORT), {}),
        "RCXB blksort 2 bytes more": ("header_bytes", (0, 32768, 32768, [0, 9, 11], c.FLAG_BLKSORT), {}),
        "RCXB crcs": ("header_bytes", (2, 16, 40, [0, 5, 12, 20]), {"crcs": [1, 2, 0xFFFFFFFF]}),
        "RCXB crcs and the flag": ("header_bytes", (2, 16, 40, [0, 5, 12, 20], c.FLAG_CRC32), {"crcs": [1, 2, 3]}),
        "RCXB stored none": ("header_bytes", (3, 16, 40, [0, 5, 12, 20]), {"stored": [0, 0, 0]}),
        "RCXB stored some": ("header_bytes", (0, 16, 40, [0, 5, 21, 29]), {"stored": [0, 1, 0]}),
        "RCXB stored last, crcs, blksort": ("header_bytes", (0, 16, 40, [0, 5, 12, 20], c.FLAG_BLKSORT), {"crcs": [1, 2, 3], "stored": [False, False, True]}),
        "RCXB nine blocks stored": ("header_bytes", (0, 16, 144, list(range(0, 145, 16))), {"stored": [1] * 9}),
        "RCXB no blocks": ("header_bytes", (0, 16, 0, [0]), {}),
        "RCXB no blocks, crcs": ("header_bytes", (0, 16, 0, [0]), {"crcs": []}),
        "RCXB no blocks, stored": ("header_bytes", (0, 16, 0, [0]), {"stored": []}),
        "RCXB refuses the stored flag": ("header_bytes", (0, 16, 40, [0, 5, 12, 20], c.FLAG_STORED), {}),
        "RCXB refuses the offsets": ("header_bytes", (0, 16, 40, [0, 5, 12]), {}),
        "RCXB refuses the offsets, blksort": ("header_bytes", (0, 32768, 32768, [0, 9], c.FLAG_BLKSORT), {}),
        "RCXB refuses stored of the wrong length": ("header_bytes", (0, 16, 40, [0, 5, 12, 20]), {"stored": [0, 1]}),
        "RCXB refuses a stored block of the wrong size": ("header_bytes", (0, 16, 40, [0, 5, 12, 20]), {"stored": [0, 1, 0]}),
        "RCXB refuses a stored last block of the wrong size": ("header_bytes", (0, 16, 40, [0, 5, 12, 28]), {"stored": [0, 0, 1]}),
        "RCXB refuses the flag without checksums": ("header_bytes", (0, 16, 40, [0, 5, 12, 20], c.FLAG_CRC32), {}),
        "RCXB refuses too few checksums": ("header_bytes", (0, 16, 40, [0, 5, 12, 20]), {"crcs": [1, 2]}),
        "RCXB stored of the wrong length before the checksums": ("header_bytes", (0, 16, 40, [0, 5, 12, 20]), {"crcs": [1], "stored": [1]}),
        # RCXI
        "RCXI plain": ("item_header_bytes", (1, [3, 0, 7], [0, 2, 2, 9]), {}),
        "RCXI crcs": ("item_header_bytes", (0, [3, 0, 7], [0, 2, 2, 9]), {"crcs": [7, 0, 9]}),
        "RCXI empty items": ("item_header_bytes", (0, [0, 0], [0, 0, 0]), {"crcs": [0, 0]}),
        "RCXI no items": ("item_header_bytes", (2, [], [0]), {}),
        "RCXI no items, crcs": ("item_header_bytes", (2, [], [0]), {"crcs": []}),
        "RCXI refuses the offsets": ("item_header_bytes", (0, [3, 0, 7], [0, 2, 2]), {}),
        "RCXI refuses a long item": ("item_header_bytes", (0, [3, big], [0, 2, 9]), {}),
        "RCXI refuses too many checksums": ("item_header_bytes", (0, [3, 0, 7], [0, 2, 2, 9]), {"crcs": [1, 2, 3, 4]}),
        # RCXT
        "RCXT plain": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {}),
        "RCXT crcs": ("typed_header_bytes", (1, 16, 40, 4, [0, 5, 12, 20], [1, 2, 3]), {}),
        "RCXT pred 1": ("typed_header_bytes", (2, 16, 40, 8, [0, 5, 12, 20]), {"pred": 1}),
        "RCXT pred 2, crcs": ("typed_header_bytes", (3, 16, 40, 4, [0, 5, 12, 20], [1, 2, 3], 2), {}),
        "RCXT stored none, pred 1": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {"pred": 1, "stored": [0, 0, 0]}),
        "RCXT version 3, pred 0": ("typed_header_bytes", (0, 16, 40, 8, [0, 5, 21, 29]), {"stored": [0, 1, 0]}),
        "RCXT version 3, pred 2, crcs": ("typed_header_bytes", (0, 16, 40, 8, [0, 5, 21, 29], [1, 2, 3], 2, [0, 1, 0]), {}),
        "RCXT no blocks": ("typed_header_bytes", (0, 16, 0, 2, [0]), {}),
        "RCXT no blocks, crcs, pred 1": ("typed_header_bytes", (0, 16, 0, 2, [0], [], 1), {}),
        "RCXT refuses the width": ("typed_header_bytes", (0, 16, 40, 3, [0, 5, 12, 20]), {}),
        "RCXT refuses width 1": ("typed_header_bytes", (0, 16, 40, 1, [0, 5, 12, 20]), {}),
        "RCXT refuses pred 3": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {"pred": 3}),
        "RCXT refuses pred True": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {"pred": True}),
        "RCXT refuses the width before the pred": ("typed_header_bytes", (0, 16, 40, 5, [0, 5, 12]), {"pred": 7}),
        "RCXT refuses the offsets": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12]), {}),
        "RCXT refuses too few checksums": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20], [1]), {}),
        "RCXT refuses stored of the wrong length": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {"stored": [1, 0, 0, 0]}),
        "RCXT refuses a stored block of the wrong size": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20]), {"stored": [1, 0, 0]}),
        "RCXT too few checksums before stored of the wrong length": ("typed_header_bytes", (0, 16, 40, 2, [0, 5, 12, 20], [1]), {"stored": [1]}),
        # RCXJ
        "RCXJ plain": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], None, [0, 3, 3, 3, 4, 5, 6, 8]), {}),
        "RCXJ crcs, preds, directory": ("typed_items_header_bytes", (1, [5, 0, 9], [1, 2, 4], [0, 1, 2], [0, 3, 3, 3, 4, 5, 6, 8], [1, 0, 0, 4, 5, 6, 7], b"dir"), {}),
        "RCXJ directory only": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], None, [0, 3, 3, 3, 4, 5, 6, 8]), {"directory": bytearray(b"\x00\xff")}),
        "RCXJ empty items": ("typed_items_header_bytes", (0, [0, 0], [2, 8], [1, 0], [0] * 11, [0] * 10), {}),
        "RCXJ no items": ("typed_items_header_bytes", (3, [], [], None, [0]), {}),
        "RCXJ no items, crcs, directory": ("typed_items_header_bytes", (3, [], [], [], [0], [], b"[]"), {}),
        "RCXJ refuses the tables": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2], None, [0, 3, 3, 3]), {}),
        "RCXJ refuses the preds' length": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], [0, 0], [0, 3, 3, 3, 4, 5, 6, 8]), {}),
        "RCXJ refuses a width": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 3, 4], None, [0, 3, 3, 3, 4, 5, 6, 8]), {}),
        "RCXJ refuses a pred": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], [0, 3, 0], [0, 3, 3, 3, 4, 5, 6, 8]), {}),
        "RCXJ refuses a pred at width 1": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], [1, 0, 0], [0, 3, 3, 3, 4, 5, 6, 8]), {}),
        "RCXJ refuses a long sub-item": ("typed_items_header_bytes", (0, [2 * big], [2], None, [0, 1, 2]), {}),
        "RCXJ refuses the offsets": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], None, [0, 3, 3, 3, 4, 5, 6]), {}),
        "RCXJ refuses too few checksums": ("typed_items_header_bytes", (0, [5, 0, 9], [1, 2, 4], None, [0, 3, 3, 3, 4, 5, 6, 8], [1, 2, 3]), {}),
    }


def valid_blobs():
    """name -> (layout, blob): tiny containers of every version and option, with payloads nobody decodes."""
    sets = header_sets()

    def blob(name, size, salt):
        writer, args, kwargs = sets[name]
        return getattr(container, writer)(*args, **kwargs) + _payload(size, salt)

    return {
        "RCXB plain": ("RCXB", blob("RCXB plain", 20, 1)),
        "RCXB crcs": ("RCXB", blob("RCXB crcs", 20, 2)),
        "RCXB stored": ("RCXB", blob("RCXB stored some", 29, 3)),
        "RCXB stored, crcs, blksort": ("RCXB", blob("RCXB stored last, crcs, blksort", 20, 4)),
        "RCXB nine stored": ("RCXB", blob("RCXB nine blocks stored", 144, 5)),
        "RCXI plain": ("RCXI", blob("RCXI plain", 9, 6)),
        "RCXI crcs": ("RCXI", blob("RCXI crcs", 9, 7)),
        "RCXT plain": ("RCXT", blob("RCXT plain", 20, 8)),
        "RCXT crcs": ("RCXT", blob("RCXT crcs", 20, 9)),
        "RCXT pred 2, crcs": ("RCXT", blob("RCXT pred 2, crcs", 20, 10)),
        "RCXT version 3, pred 0": ("RCXT", blob("RCXT version 3, pred 0", 29, 11)),
        "RCXT version 3, pred 2, crcs": ("RCXT", blob("RCXT version 3, pred 2, crcs", 29, 12)),
        "RCXJ plain": ("RCXJ", blob("RCXJ plain", 8, 13)),
        "RCXJ crcs, preds, directory": ("RCXJ", blob("RCXJ crcs, preds, directory", 8, 14)),
        "RCXJ directory only": ("RCXJ", blob("RCXJ directory only", 8, 15)),
    }


def damaged(layout: str, blob: bytes):
    """The damaged forms of one valid blob, in a fixed order -> [(what, bytes)]: every byte of the fixed part set to 0, to 0xFF
    and to its value + 1; every byte of the tables raised by 1; the blob cut at every length up to the end of the tables; one byte
    more behind it."""
    tables = len(blob) - len(getattr(container, PARSERS[layout])(blob)["payload"])
    out = []
    for at in range(FIXED[layout]):
        for what, v in (("=00", 0), ("=ff", 0xFF), ("+1", (blob[at] + 1) & 0xFF)):
            out.append((f"byte {at} {what}", blob[:at] + bytes([v]) + blob[at + 1:]))
    for at in range(FIXED[layout], tables):
        out.append((f"byte {at} +1", blob[:at] + bytes([(blob[at] + 1) & 0xFF]) + blob[at + 1:]))
    for cut in range(tables + 1):
        out.append((f"cut at {cut}", blob[:cut]))
    out.append(("one byte more", blob + b"\x00"))
    return out


def parser_verdicts():
    """name of a valid blob -> {"blob": hex, "parsed": the parser's result, "verdicts": the distinct verdicts, "damaged": [[what,
    index into verdicts]]}.  Every other parser refuses the blob too: "foreign"."""
    out = {}
    for name, (layout, blob) in valid_blobs().items():
        parser = getattr(container, PARSERS[layout])
        verdicts, rows = [], []
        for what, bad in damaged(layout, blob):
            v = verdict(parser, bad)
            if v not in verdicts:
                verdicts.append(v)
            rows.append([what, verdicts.index(v)])
        foreign = {other: verdict(getattr(container, PARSERS[other]), blob) for other in PARSERS if other != layout}
        as_array = verdict(parser, np.frombuffer(blob, np.uint8))
        out[name] = {"blob": blob.hex(), "parsed": plain(parser(blob)), "as_array": as_array, "foreign": foreign, "verdicts": verdicts, "damaged": rows}
    return out


def directory_results():
    c = container
    entries = [{"name": "a", "dtype": "int64", "shape": (3, 7), "first": 0, "count": 2}, {"name": "b", "dtype": "float16", "shape": (), "first": 2, "count": 0}]
    good = c.tensor_directory_bytes(entries)
    texts = {"good": good, "not JSON": b"\xff{", "not a list": b"{}", "a key short": b'[{"name":"a","dtype":"u","shape":[1],"first":0}]',
             "an entry that is no dict": b"[1]", "past the items": good.replace(b'"count":2', b'"count":4'),
             "negative first": good.replace(b'"first":0', b'"first":-1'), "negative shape": good.replace(b"[3,7]", b"[3,-7]"),
             "a name twice": good.replace(b'"name":"b"', b'"name":"a"'), "empty": b"[]", "empty bytes": b""}
    return {"bytes": good.hex(), "parsed": {k: outcome(c.parse_tensor_directory, v, 3) for k, v in texts.items()}}


def no_gpu_returns():
    """What pack and unpack give where there is nothing to code or decode: no context is made, so no library is needed."""
    c = container
    typed = c.pack_typed(b"", width=2)
    typed_crc = c.pack_typed(np.zeros(0, np.uint32), checksum=True, predict="auto")
    items = c.pack_typed_items([b"", b""], widths=2)
    items_crc = c.pack_typed_items([b"", np.zeros(0, np.int64)], widths=[1, 8], predict=[None, "delta"], checksum=True, directory=b"d")
    import torch
    tensors = c.pack_tensors({"e": torch.zeros(0, dtype=torch.float16)})
    rcxb = valid_blobs()["RCXB plain"][1]
    rcxt = valid_blobs()["RCXT plain"][1]
    rcxi = valid_blobs()["RCXI plain"][1]
    return {
        "pack_typed empty": typed.hex(), "pack_typed empty, crcs, auto": typed_crc.hex(), "unpack_typed empty": outcome(c.unpack_typed, typed),
        "unpack_typed_range empty": outcome(c.unpack_typed_range, typed, 0, 0),
        "pack_typed_items empty": items.hex(), "pack_typed_items empty, crcs": items_crc.hex(),
        "unpack_typed_items empty": outcome(c.unpack_typed_items, items), "unpack_typed_items empty, crcs": outcome(c.unpack_typed_items, items_crc, [1, 0, 1]),
        "unpack_typed_items no picks": outcome(c.unpack_typed_items, items, pick=[]),
        "unpack_typed_items no such item": outcome(c.unpack_typed_items, items, pick=[2]),
        "pack_tensors empty": tensors.hex(), "pack_tensors empty numpy": outcome(c.pack_tensors, {"e": np.zeros(0, np.float16)}),
        "unpack_tensors empty": outcome(c.unpack_tensors, tensors), "unpack_tensors no names": outcome(c.unpack_tensors, tensors, names=[]),
        "unpack_tensors no such tensor": outcome(c.unpack_tensors, tensors, names=["f"]),
        "unpack_range empty": outcome(c.unpack_range, rcxb, 3, 3), "unpack_range outside": outcome(c.unpack_range, rcxb, 3, 41),
        "unpack_range blksort": outcome(c.unpack_range, valid_blobs()["RCXB stored, crcs, blksort"][1], 0, 1),
        "unpack_typed_range empty range": outcome(c.unpack_typed_range, rcxt, 7, 7), "unpack_typed_range outside": outcome(c.unpack_typed_range, rcxt, 8, 7),
        "unpack_items no picks": outcome(c.unpack_items, rcxi, pick=[]), "unpack_items no such item": outcome(c.unpack_items, rcxi, pick=[3]),
        "unpack no bytes": outcome(c.unpack, c.header_bytes(0, 16, 0, [0])),
        "refusals": {
            "pack_typed plain bytes": outcome(c.pack_typed, b"abcd"), "pack_typed width 3": outcome(c.pack_typed, b"abcd", width=3),
            "pack_typed width 1 array": outcome(c.pack_typed, np.zeros(4, np.uint8)), "pack_typed predictor": outcome(c.pack_typed, b"", width=2, predict="xor"),
            "pack_typed stored": outcome(c.pack_typed, b"", width=2, stored=1.5), "pack stored": outcome(c.pack, b"", stored="yes"),
            "pack_typed_items plain bytes": outcome(c.pack_typed_items, [b"ab", np.zeros(1, np.int16)]),
            "pack_typed_items widths": outcome(c.pack_typed_items, [b"ab"], widths=[2, 2]), "pack_typed_items width 3": outcome(c.pack_typed_items, [b"ab"], widths=3),
            "pack_typed_items predictors": outcome(c.pack_typed_items, [b""], widths=2, predict=["delta", None]),
            "pack_typed_items predictor at width 1": outcome(c.pack_typed_items, [b""], widths=1, predict=["delta"]),
            "pack_typed_items predictor name": outcome(c.pack_typed_items, [b""], widths=2, predict="xor"),
            "pack_tensors block": outcome(c.pack_tensors, {"e": np.zeros(0, np.float16)}, block=8), "pack_tensors bytes": outcome(c.pack_tensors, {"e": b""}),
            "pack_tensors complex": outcome(c.pack_tensors, {"e": np.zeros(2, np.complex128)}),
        },
    }


def _delta_blobs():
    """Tiny RCXK containers with payloads nobody decodes -> (one of plain items, one of tensors "a", "e", "z")."""
    c = container
    ops, offsets = [0, c.BASE_OP_NONE, 2], [0, 3, 3, 3, 4, 5, 6, 8]
    directory = c.tensor_directory_bytes([{"name": "a", "dtype": "uint8", "shape": (5,), "first": 0, "count": 1}, {"name": "e", "dtype": "int16", "shape": (0,),
    "first": 1, "count": 1},
                                          {"name": "z", "dtype": "int32", "shape": (2,), "first": 2, "count": 1}, {"name": "u", "dtype": "u", "shape": (0,),
                                          "first": 3, "count": 0}])
    items = c.delta_items_header_bytes(ops, [7, 0, 9]) + c.typed_items_header_bytes(0, [5, 0, 8], [1, 2, 4], None, offsets) + _payload(8, 21)
    tensors = c.delta_items_header_bytes(ops) + c.typed_items_header_bytes(0, [5, 0, 8], [1, 2, 4], None, offsets, None, directory) + _payload(8, 22)
    return items, tensors


def delta_no_gpu_returns():
    """The same for the containers against a base: what returns or is refused before a context exists."""
    import torch
    c = container
    e16, e8 = np.zeros(0, np.int16), b""
    a, b = np.arange(6, dtype=np.int16), np.arange(6, dtype=np.int16) + 1
    rcxd = c.pack_delta(e8, e8, width=2)
    rcxd_crc = c.pack_delta(e16, e16, checksum=True, op="auto", base_check=False)
    rcxk = c.pack_delta_items([e8, e16], [e8, None], widths=[1, 2], ops=["xor", None], predict=[None, "delta"], checksum=True, directory=b"d")
    rcxk_auto = c.pack_delta_items([e8, e16], [e8, e16], widths=2, ops=["auto", "auto"], predict="auto", base_check=False)
    named, base = {"e": torch.zeros(0, dtype=torch.float16), "f": torch.zeros((0, 3), dtype=torch.int32)}, {"e": torch.zeros(0, dtype=torch.float16)}
    tensors = c.pack_tensors_delta(named, base)
    items_blob, tensors_blob = _delta_blobs()
    some = [b"12345", None, b"12345678"]
    return {
        "pack_delta empty": rcxd.hex(), "pack_delta empty, crcs, auto, no guard": rcxd_crc.hex(),
        "pack_delta empty width 1": outcome(c.pack_delta, e8, e8, width=1, stored=True),
        "unpack_delta empty": outcome(c.unpack_delta, rcxd, e8), "unpack_delta_range empty": outcome(c.unpack_delta_range, rcxd_crc, e8, 0, 0),
        "pack_delta_items empty": rcxk.hex(), "pack_delta_items empty, auto": rcxk_auto.hex(), "pack_delta_items no items": outcome(c.pack_delta_items, [], []),
        "choose_delta_items empty": outcome(c.choose_delta_items, [e8, e16], [e8, e16], widths=2, ops=["auto", None], predict="auto"),
        "unpack_delta_items empty": outcome(c.unpack_delta_items, rcxk, [None, None]),
        "unpack_delta_items empty picks": outcome(c.unpack_delta_items, rcxk, [None, None], pick=[1, 0, 1]),
        "unpack_delta_items no picks": outcome(c.unpack_delta_items, items_blob, some, pick=[]),
        "unpack_delta_items an empty item": outcome(c.unpack_delta_items, items_blob, [None] * 3, pick=[1]),
        "pack_tensors_delta empty": tensors.hex(), "pack_tensors_delta empty, auto": outcome(c.pack_tensors_delta, named, base, op="auto", predict="auto", checksum=True),
        "choose_tensors_delta empty": outcome(c.choose_tensors_delta, named, base), "unpack_tensors_delta empty": outcome(c.unpack_tensors_delta, tensors, {}),
        "unpack_tensors_delta no names": outcome(c.unpack_tensors_delta, tensors_blob, {}, names=[]),
        "unpack_tensors_delta an empty tensor": outcome(c.unpack_tensors_delta, tensors_blob, {}, names=["e"]),
        "refusals": {
            "pack_delta op": outcome(c.pack_delta, a, b, op="and"), "pack_delta op 2": outcome(c.pack_delta, a, b, op=2),
            "pack_delta plain bytes": outcome(c.pack_delta, b"abcd", b"abcd"),
            "pack_delta width 3": outcome(c.pack_delta, a, b, width=3), "pack_delta base length": outcome(c.pack_delta, a, b[:5]),
            "pack_delta stored": outcome(c.pack_delta, a, b, stored=1.0),
            "pack_delta the op before the width": outcome(c.pack_delta, a, b[:5], width=3, op="or"),
            "pack_delta the width before the base": outcome(c.pack_delta, a, b[:5], width=3),
            "pack_delta block": outcome(c.pack_delta, e16, e16, block=8),
            "unpack_delta base length": outcome(c.unpack_delta, rcxd, b"ab"), "unpack_delta_range base length": outcome(c.unpack_delta_range, rcxd, b"ab", 0, 0),
            "unpack_delta_range outside": outcome(c.unpack_delta_range, rcxd, e8, 0, 1),
            "pack_delta_items bases": outcome(c.pack_delta_items, [a, a], [b]),
            "pack_delta_items bases, auto": outcome(c.pack_delta_items, [a, a], [b], ops=["auto", None]),
            "pack_delta_items plain bytes": outcome(c.pack_delta_items, [b"ab", a], [None, b]),
            "pack_delta_items widths": outcome(c.pack_delta_items, [a], [b], widths=[2, 2]),
            "pack_delta_items width 3": outcome(c.pack_delta_items, [a], [b], widths=3),
            "pack_delta_items width 3, auto": outcome(c.pack_delta_items, [a], [b], widths=3, ops=["auto"]),
            "pack_delta_items base length": outcome(c.pack_delta_items, [a, a], [b, b[:5]]),
            "pack_delta_items base length, auto": outcome(c.pack_delta_items, [a, a], [b, b[:5]], ops=["auto", "xor"]),
            "pack_delta_items ops": outcome(c.pack_delta_items, [a, a], [b, b], ops=["xor"]),
            "pack_delta_items ops, auto": outcome(c.pack_delta_items, [a, a], [b, b], ops=["auto"]),
            "pack_delta_items op name": outcome(c.pack_delta_items, [a], [b], ops="and"),
            "pack_delta_items op name in a list": outcome(c.pack_delta_items, [a, a], [b, b], ops=["and", "auto"]),
            "pack_delta_items op auto for all": outcome(c.pack_delta_items, [a], [b], ops="auto"),
            "pack_delta_items op 2": outcome(c.pack_delta_items, [a], [b], ops=[2]),
            "pack_delta_items op without a base": outcome(c.pack_delta_items, [a, a], [b, None], ops=["xor", "sub"]),
            "pack_delta_items op without a base, auto": outcome(c.pack_delta_items, [a, a], [b, None], ops=["auto", "sub"]),
            "pack_delta_items auto without a base": outcome(c.pack_delta_items, [a, a], [b, None], ops=["xor", "auto"]),
            "pack_delta_items predictors": outcome(c.pack_delta_items, [a, a], [b, None], ops=["xor", None], predict=[None]),
            "pack_delta_items predictors, auto": outcome(c.pack_delta_items, [a, a], [b, None], ops=["auto", None], predict=[None]),
            "pack_delta_items predictor with a base": outcome(c.pack_delta_items, [a, a], [b, None], ops=["xor", None], predict=["delta", None]),
            "pack_delta_items predictor with a base, auto": outcome(c.pack_delta_items, [a, a], [b, None], ops=["auto", None], predict=["delta", None]),
            "pack_delta_items predictor name": outcome(c.pack_delta_items, [a, a], [b, None], ops=["xor", None], predict="xor"),
            "pack_delta_items predictor name, auto": outcome(c.pack_delta_items, [a, a], [b, None], ops=["auto", None], predict=[None, "xor"]),
            "pack_delta_items predictor at width 1": outcome(c.pack_delta_items, [b"ab", a], [b"cd", None], widths=[1, 2], ops=["xor", None],
                                                             predict=["delta", None]),
            "pack_delta_items stored": outcome(c.pack_delta_items, [a], [b], stored=-1),
            "choose_delta_items bases": outcome(c.choose_delta_items, [a, a], [b]), "choose_delta_items op name": outcome(c.choose_delta_items, [a], [b], ops="and"),
            "unpack_delta_items bases": outcome(c.unpack_delta_items, items_blob, some[:2]),
            "unpack_delta_items no such item": outcome(c.unpack_delta_items, items_blob, some, pick=[3]),
            "unpack_delta_items no base": outcome(c.unpack_delta_items, items_blob, [None] * 3),
            "unpack_delta_items base length": outcome(c.unpack_delta_items, items_blob, [b"1234", None, None], pick=[1, 0]),
            "unpack_delta_items no base of the second": outcome(c.unpack_delta_items, items_blob, [b"12345", None, None]),
            "pack_tensors_delta block 8": outcome(c.pack_tensors_delta, named, base, block=8),
            "pack_tensors_delta block": outcome(c.pack_tensors_delta, named, base, block=c.MAX_ITEM + 1),
            "pack_tensors_delta the block before the op": outcome(c.pack_tensors_delta, named, base, block=8, op={"f": "xor"}),
            "pack_tensors_delta dict op, no base": outcome(c.pack_tensors_delta, named, base, op={"f": "xor"}),
            "pack_tensors_delta dict op, another shape": outcome(c.pack_tensors_delta, named, {"f": torch.zeros((3, 0), dtype=torch.int32)}, op={"f": "auto"}),
            "pack_tensors_delta dict op, another dtype": outcome(c.pack_tensors_delta, named, {"f": torch.zeros((0, 3), dtype=torch.int64)}, op={"e": None, "f": "sub"}),
            "pack_tensors_delta dict op, a name that is no tensor": outcome(c.pack_tensors_delta, named, base, op={"g": "xor", "e": "xor"}),
            "pack_tensors_delta bytes": outcome(c.pack_tensors_delta, {"e": b""}, {}),
            "pack_tensors_delta bytes in the base": outcome(c.pack_tensors_delta, named, {"e": b""}),
            "pack_tensors_delta bytes under a dict op": outcome(c.pack_tensors_delta, {"e": b""}, {"e": b""}, op={"e": "xor"}),
            "pack_tensors_delta complex": outcome(c.pack_tensors_delta, {"e": np.zeros(2, np.complex128)}, {}),
            "pack_tensors_delta op name": outcome(c.pack_tensors_delta, {"t": a}, {"t": b}, op="and"),
            "pack_tensors_delta predictor name": outcome(c.pack_tensors_delta, {"t": a}, {}, predict={"t": "xor"}),
            "pack_tensors_delta stored": outcome(c.pack_tensors_delta, named, base, stored="yes"),
            "pack_tensors_delta auto, bytes": outcome(c.pack_tensors_delta, {"e": b""}, {}, op="auto"),
            "unpack_tensors_delta no such tensor": outcome(c.unpack_tensors_delta, tensors_blob, {}, names=["f"]),
            "unpack_tensors_delta dtype": outcome(c.unpack_tensors_delta, tensors_blob, {}, names=["u"]),
            "unpack_tensors_delta no base": outcome(c.unpack_tensors_delta, tensors_blob, {}, names=["e", "a"]),
            "unpack_tensors_delta base size": outcome(c.unpack_tensors_delta, tensors_blob, {"a": np.zeros(4, np.uint8), "z": np.zeros(2, np.int32)}, names=["z", "a"]),
            "unpack_tensors_delta base that is bytes": outcome(c.unpack_tensors_delta, tensors_blob, {"a": b"12345"}, names=["a"]),
        },
    }


def decisions():
    """The rules of "auto" on small tables: the margin of 1/64 on both sides and every tie."""
    import torch
    c = container
    tables = ([6400, 6300, 6300, 6300, 6300, 6300], [6400, 6299, 6299, 6299, 6299, 6299], [6400, 6300, 6299, 6299, 6299, 6299], [6400, 6300, 6300, 6299, 6299, 6299],
              [6400, 6300, 6300, 6299, 6299, 6300], [6400, 6300, 6300, 6299, 6300, 6300], [6400, 6299, 6298, 6299, 6299, 6299], [6400, 100, 100, 99, 100, 100],
              [6400, 6400, 6400, 6400, 6400, 98], [0, 0, 0, 0, 0, 0], [64, 62, 63, 62, 62, 62], [64, 63, 62, 61, 61, 61])
    has_base, widths = [True, True, False, True, False, True], [1, 2, 4, 8, 1, 2]
    costs = [[100, 90, 90, 50, 50, 50], [100, 40, 40, 50, 50, 50], [100, 99, 98, 1, 1, 1], [100, 99, 99, 99, 99, 99], [100, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]]
    forms = {"auto": ("auto", None), "auto, auto": ("auto", "auto"), "auto, delta": ("auto", "delta"), "subzz, auto": ("subzz", "auto"),
             "lists": (["auto", "xor", None, "auto", None, None], [None, None, "auto", "auto", None, "zigzag"]),
             "None, lists": (None, [None, "delta", "auto", None, None, "auto"]),
             "a named predictor on an auto op": (["auto"] * 2 + [None] + ["auto"] + [None, "sub"], [None, "delta", None, None, None, None]),
             "auto without a base": (["auto", None, "auto", None, None, None], None), "ops too few": (["auto"], None), "predictors too few": ("auto", [None]),
             "an op name": (["and"] + [None] * 5, None), "a predictor name": ("auto", "xor")}
    named = {"a": np.arange(40, dtype=np.int16), "b": torch.zeros(0, dtype=torch.float32), "c": np.arange(5, dtype=np.uint8), "d": np.zeros((3, 7), np.float32),
    "e": np.arange(24, dtype=np.int64)}
    base = {"a": np.arange(40, dtype=np.int16) + 1, "c": np.zeros(5, np.uint8), "d": np.zeros((7, 3), np.float32), "e": np.zeros(24, np.int64),
    "g": np.zeros(3, np.uint8)}
    tensor_forms = {"auto": ("auto", None), "auto, auto": ("auto", "auto"), "dicts": ({"a": "auto", "c": "xor", "e": None}, {"e": "auto", "d": "delta"}),
    "subzz, dict": ("subzz", {"d": "auto"}),
                    "an op name": ("and", None), "a predictor name": ("auto", {"a": "auto", "d": "xor"})}
    out = {"CANDIDATES": list(c.CANDIDATES),
           "pick_candidate": [[t, asked, outcome(c.pick_candidate, t, asked)] for t in tables for asked in (0x3F, 0x39, 0x07)] + [[tables[0], 0x3E, outcome(c.pick_candidate, tables[0], 0x3E)]],
           "pick_candidate all asked": [[t, outcome(c.pick_candidate, t)] for t in tables[:3]],
           "pick_op": [[t, c.pick_op(*t)] for t in ((5, 5, 5), (4, 5, 5), (5, 4, 5), (5, 5, 4), (4, 4, 5), (4, 5, 4), (5, 4, 4), (0, 0, 0), (3, 2, 1), (1, 2, 3))],
           "delta_item_masks": {k: outcome(c.delta_item_masks, has_base, widths, ops=o, predict=p) for k, (o, p) in forms.items()},
           "choose_delta_items_from_costs": {k: outcome(c.choose_delta_items_from_costs, costs, has_base, widths, ops=o, predict=p) for k, (o, p) in forms.items()},
           "tensor_delta_masks": {k: outcome(c.tensor_delta_masks, named, base, block=16, op=o, predict=p) for k, (o, p) in tensor_forms.items()}}
    nitems = len(c.tensor_delta_masks(named, base, block=16)["lengths"])
    for tag, rows in (("ops win", [[1000, 990, 990, 300, 200, 200]] * nitems), ("none wins", [[1000, 990, 990, 990, 990, 990]] * nitems),
                      ("a tensor decides on its sums", [[1000, 990, 990, 100 + 900 * (i % 2), 985, 985] for i in range(nitems)])):
        out[f"choose_tensors_delta_from_costs, {tag}"] = {k: outcome(c.choose_tensors_delta_from_costs, rows, named, base, block=16, op=o, predict=p)
                                                          for k, (o, p) in tensor_forms.items()}
    return out


def public_names():
    """The sorted public names of `container` that are no modules."""
    return sorted(k for k, v in vars(container).items() if not k.startswith("_") and not isinstance(v, types.ModuleType))


def cpu_section():
    c = container
    sets = header_sets()
    no_gpu, more = no_gpu_returns(), delta_no_gpu_returns()
    assert not set(no_gpu) & (set(more) - {"refusals"}) and not set(no_gpu["refusals"]) & set(more["refusals"])
    no_gpu = no_gpu | more | {"refusals": no_gpu["refusals"] | more["refusals"]}
    return {
        "constants": plain({k: getattr(c, k) for k in CONSTANTS} | {"PREDICTORS": {str(k): v for k, v in c.PREDICTORS.items()}}),
        "coded_size": [[n, f, c.coded_size(n, f)] for n in (0, 1, 32767, 32768, 65535, 65536, 1 << 20) for f in (0, 1, 2, 3, 7)],
        "pick_predictor": [[a, b, d, c.pick_predictor(a, b, d)]
                           for a, b, d in ((6400, 6300, 6300), (6400, 6299, 6299), (6400, 6299, 6298), (6400, 6400, 100), (0, 0, 0), (64, 62, 63))],
        "errors": plain([str(c.ChecksumError("block", np.int64(7))), c.ChecksumError("item", 3).index, issubclass(c.ChecksumError, c.ContainerError),
                         issubclass(c.ContainerError, ValueError)]),
        "headers": {name: outcome(getattr(c, writer), *args, **kwargs) for name, (writer, args, kwargs) in sets.items()},
        "parsers": parser_verdicts(),
        "directory": directory_results(),
        "no_gpu": no_gpu,
        "decisions": decisions(),
        "names": public_names(),
    }


# ---- the GPU section: blobs and call traces --------------------------------------------------------------------------------------
DEVICE_CALLS = ("stored.mix_device", "stored.decode_device", "predict.split_device", "predict.join_device", "typed_items.split_device", "typed_items.join_device",
                "stats.blocks_device", "stats.items_device", "stored_items.mix_items_device", "base.split_device", "base.join_device",
                "base_items.split_device", "base_items.join_device", "typed_stats.items_device", "picks.reserve", "picks.decode_device",
                "typed_picks.reserve", "typed_picks.join_device")
COPIES = ("cuda", "cpu")  # the torch.Tensor methods that move bytes between host and device


def _logged(log, name, fn):
    def call(*args, **kwargs):
        if name != "close" or getattr(args[0], "_h", None):  # (a close that destroys a context: the one from __del__ behind it is none)
            log.append(name)
        return fn(*args, **kwargs)
    return call


class Recorder:
    """Keeps, per labelled public call, the names of the rcx.Context methods and module device calls made inside it, in order,
    and beside them ("copies") the names of the torch.Tensor.cuda and .cpu calls.
    install(setattr) puts the recording wrappers in place through the caller's setattr(target, name, value) -- a test's
    monkeypatch.setattr -- which is also what takes them out again."""

    def __init__(self):
        self.log, self.moved, self.record = [], [], {"traces": {}, "copies": {}}

    def install(self, setattr_):
        import importlib
        from cpprcoder_amd import rcx
        for name, fn in list(vars(rcx.Context).items()):
            if isinstance(fn, types.FunctionType) and not name.startswith("_"):
                setattr_(rcx.Context, name, _logged(self.log, name, fn))
        for dotted in DEVICE_CALLS:
            module, name = dotted.split(".")
            mod = importlib.import_module("cpprcoder_amd." + module)
            setattr_(mod, name, _logged(self.log, dotted, getattr(mod, name)))
        import torch
        for name in COPIES:
            setattr_(torch.Tensor, name, _logged(self.moved, name, getattr(torch.Tensor, name)))

    def call(self, label, fn, *args, **kwargs):
        del self.log[:], self.moved[:]
        try:
            return fn(*args, **kwargs)
        finally:
            assert label not in self.record["traces"], label
            self.record["traces"][label] = list(self.log)
            self.record["copies"][label] = list(self.moved)

    def blob(self, label, fn, *args, **kwargs):
        b = self.call(label, fn, *args, **kwargs)
        self.record.setdefault("blobs", {})[label] = {"sha256": hashlib.sha256(b).hexdigest(), "len": len(b)}
        return b

    def note(self, key, value):
        self.record.setdefault("values", {})[key] = plain(value)


@contextlib.contextmanager
def recording():
    """A Recorder whose wrappers are in place inside the block (for the maker; a test hands install() its monkeypatch.setattr)."""
    saved, rec = [], Recorder()

    def setattr_(target, name, value):
        saved.append((target, name, getattr(target, name)))
        setattr(target, name, value)

    rec.install(setattr_)
    try:
        yield rec
    finally:
        for target, name, value in reversed(saved):
            setattr(target, name, value)


def _bytes(seed: int, n: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, n, dtype=np.uint8)


def _sorted_ints(seed: int, width: int, count: int) -> np.ndarray:
    """`count` sorted unsigned integers of `width` bytes with small steps: something for a predictor to earn."""
    steps = np.random.RandomState(seed).randint(0, 3, count).astype(np.uint64)
    return (np.cumsum(steps) + np.uint64(250)).astype({1: np.uint8, 2: "<u2", 4: "<u4", 8: "<u8"}[width])


def _typed_bytes(seed: int, width: int, n: int) -> np.ndarray:
    """n bytes: sorted integers of `width` bytes and a tail of n % width random ones."""
    return np.concatenate([_sorted_ints(seed, width, n // width).view(np.uint8), _bytes(seed + 1, n % width)])


def _noisy_low_planes(seed: int, width: int, n: int) -> np.ndarray:
    """n bytes of `width`-byte elements whose top byte climbs slowly and whose other bytes are random: planes that do not shrink."""
    x = _bytes(seed, n).copy()
    x[width - 1:: width] = (np.arange(len(x[width - 1:: width])) // 16).astype(np.uint8)
    return x


def _damaged(rec, label, blob, parsed, stream, unpack):
    """One bit of payload stream `stream` flipped, at one place after another -- its end first, where the decoder has the least
    left to run dry on -- until unpack(bad blob) raises ChecksumError; every try is recorded with what it gave, and each has a
    trace of its own -> the last bad blob."""
    offs = parsed["offsets"]
    base, lo, hi = len(blob) - len(parsed["payload"]), int(offs[stream]), int(offs[stream + 1])
    assert hi > lo
    places = [hi - 1 - k for k in range(10)] + [(lo + hi) // 2, lo + (hi - lo) // 4, lo + 3 * (hi - lo) // 4] + [lo + 6 + k for k in range(3)]
    tries, bad = [], None
    for at in dict.fromkeys(p for p in places if lo <= p < hi):
        bad = blob[:base + at] + bytes([blob[base + at] ^ 0x10]) + blob[base + at + 1:]
        try:
            rec.call(f"{label} flip {at - lo}", unpack, bad)
            tries.append([at - lo, "no error"])
        except container.ChecksumError as e:
            tries.append([at - lo, {"error": type(e).__name__, "kind": e.kind, "index": e.index, "text": str(e)}])
            break
        except Exception as e:  # noqa: BLE001 (a stream that runs dry is the decoder's own error, the same on both sides)
            tries.append([at - lo, {"error": type(e).__name__, "text": str(e)}])
    rec.note(label, tries)
    return bad


RANGES = ((0, 1), (63, 65), (130, 197))


def _rcxb(data, block, coder, checksum, stored, blksort, own, ranges, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        raw = data.tobytes()
        blob = rec.blob("pack", container.pack, raw, block=block, coder=coder, ctx=use, blksort=blksort, checksum=checksum, stored=stored)
        c = container.parse(blob)
        rec.note("version flags stored", [blob[4], c["flags"], None if c["stored"] is None else c["stored"].astype(int)])
        assert rec.call("unpack", container.unpack, blob, ctx=use) == raw
        assert rec.call("unpack verify=False", container.unpack, blob, ctx=use, verify=False) == raw
        for a, b in ranges:
            assert rec.call(f"unpack_range {a} {b}", container.unpack_range, blob, a, b, ctx=use) == raw[a:b]
        if ranges:
            assert rec.call("unpack_range verify=False", container.unpack_range, blob, 63, 65, ctx=use, verify=False) == raw[63:65]
        if damage:
            k = 1 if c["stored"] is None else int(np.flatnonzero(c["stored"])[0])  # (a stored block cannot run dry)
            _damaged(rec, "damaged unpack", blob, c, k, lambda bad: container.unpack(bad, ctx=use))
            bad = _damaged(rec, "damaged unpack_range", blob, c, k, lambda bad: container.unpack_range(bad, 64 * k, 64 * k + 1, ctx=use))
            assert rec.call("damaged unpack_range beside it", container.unpack_range, bad, 64 * k - 64, 64 * k, ctx=use) == raw[64 * k - 64: 64 * k]
    return run


def _rcxi(checksum, own, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        flat = _bytes(31, 382) // 3
        items = [flat[a:b].tobytes() for a, b in zip(np.cumsum([0, 0, 1, 17, 300, 0]), np.cumsum([0, 1, 17, 300, 0, 64]))]
        assert [len(x) for x in items] == [0, 1, 17, 300, 0, 64]
        blob = rec.blob("pack_items", container.pack_items, items, ctx=use, checksum=checksum)
        for pick in (None, [3, 3, 0], [4]):
            want = items if pick is None else [items[k] for k in pick]
            assert rec.call(f"unpack_items {pick}", container.unpack_items, blob, pick=pick, ctx=use) == want
        assert rec.call("unpack_items verify=False", container.unpack_items, blob, ctx=use, verify=False) == items
        if damage:
            bad = _damaged(rec, "damaged unpack_items", blob, container.parse_items(blob), 3, lambda bad: container.unpack_items(bad, ctx=use))
            assert rec.call("damaged unpack_items beside it", container.unpack_items, bad, pick=[5, 1], ctx=use) == [items[5], items[1]]
    return run


def _rcxt(data, width, predict, checksum, stored, own, tensor=False, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        raw, n, sb = data.tobytes(), len(data), width * 64
        src = raw
        if tensor:
            import torch
            src = torch.from_numpy(data.view({2: np.int16, 4: np.int32, 8: np.int64}[width]).copy()).cuda()
        blob = rec.blob("pack_typed", container.pack_typed, src, width=None if tensor else width, block=64, ctx=use, checksum=checksum, predict=predict, stored=stored)
        c = container.parse_typed(blob)
        rec.note("version pred stored", [blob[4], c["pred"], None if c["stored"] is None else c["stored"].astype(int)])
        assert rec.call("unpack_typed", container.unpack_typed, blob, ctx=use) == raw
        for a, b in ((sb - 1, sb + 1), (2 * sb + 1, n), (0, n)):
            assert rec.call(f"unpack_typed_range {a} {b}", container.unpack_typed_range, blob, a, b, ctx=use) == raw[a:b]
        assert rec.call("unpack_typed_range verify=False", container.unpack_typed_range, blob, sb - 1, sb + 1, ctx=use, verify=False) == raw[sb - 1: sb + 1]
        if damage:
            _damaged(rec, "damaged unpack_typed", blob, c, width, lambda bad: container.unpack_typed(bad, ctx=use))  # the first block of the second superblock
            bad = _damaged(rec, "damaged unpack_typed_range", blob, c, width, lambda bad: container.unpack_typed_range(bad, sb, sb + 1, ctx=use))
            assert rec.call("damaged unpack_typed_range beside it", container.unpack_typed_range, bad, 0, sb, ctx=use) == raw[:sb]
    return run


J_WIDTHS, J_LENGTHS = [1, 2, 4, 8, 8], [5, 33, 0, 163, 7]


def _rcxj(predict, checksum, directory, own, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        items = [_typed_bytes(40 + i, w, n).tobytes() for i, (w, n) in enumerate(zip(J_WIDTHS, J_LENGTHS))]
        blob = rec.blob("pack_typed_items", container.pack_typed_items, items, widths=J_WIDTHS, predict=predict, ctx=use, checksum=checksum, directory=directory)
        c = container.parse_typed_items(blob)
        rec.note("preds", c["preds"])
        for pick in (None, [3, 0, 3], [2]):
            want = items if pick is None else [items[k] for k in pick]
            assert rec.call(f"unpack_typed_items {pick}", container.unpack_typed_items, blob, pick=pick, ctx=use) == want
        assert rec.call("unpack_typed_items verify=False", container.unpack_typed_items, blob, ctx=use, verify=False) == items
        if damage:
            first = int(c["sub_first"][3])
            assert int(c["sub_lengths"][first]) > 0
            bad = _damaged(rec, "damaged unpack_typed_items", blob, c, first, lambda bad: container.unpack_typed_items(bad, ctx=use))  # the low plane of item 3
            assert rec.call("damaged unpack_typed_items beside it", container.unpack_typed_items, bad, pick=[1, 4], ctx=use) == [items[1], items[4]]
    return run


def _tensors(predict, checksum, own, on_gpu=False, damage=False):
    def run(rec, ctx):
        import torch
        use = None if own else ctx
        named = {"a": _sorted_ints(51, 8, 100).view(np.int64), "b": torch.zeros(0, dtype=torch.float16), "c": _bytes(52, 50),
                 "d": np.random.RandomState(53).standard_normal((3, 7)).astype(np.float32)}
        given = {k: torch.as_tensor(v).cuda() for k, v in named.items()} if on_gpu else named
        blob = rec.blob("pack_tensors", container.pack_tensors, given, block=64, predict=predict, ctx=use, checksum=checksum)
        c = container.parse_typed_items(blob)
        rec.note("directory and preds", [c["directory"], c["preds"]])

        def same(got, names, device):
            assert list(got) == names
            for k in names:
                want = torch.as_tensor(named[k])
                assert got[k].device.type == device and got[k].dtype == want.dtype and got[k].shape == want.shape
                assert got[k].cpu().numpy().tobytes() == want.numpy().tobytes()

        same(rec.call("unpack_tensors", container.unpack_tensors, blob, ctx=use), ["a", "b", "c", "d"], "cpu")
        same(rec.call("unpack_tensors d a", container.unpack_tensors, blob, names=["d", "a"], ctx=use), ["d", "a"], "cpu")
        same(rec.call("unpack_tensors b", container.unpack_tensors, blob, names=["b"], ctx=use), ["b"], "cpu")
        same(rec.call("unpack_tensors cuda", container.unpack_tensors, blob, device="cuda", ctx=use), ["a", "b", "c", "d"], "cuda")
        same(rec.call("unpack_tensors verify=False", container.unpack_tensors, blob, ctx=use, verify=False), ["a", "b", "c", "d"], "cpu")
        if damage:
            bad = _damaged(rec, "damaged unpack_tensors", blob, c, 8 + 3, lambda bad: container.unpack_tensors(bad, ctx=use))  # "a" is items 0 and 1 of 8 planes each
            same(rec.call("damaged unpack_tensors beside it", container.unpack_tensors, bad, names=["c", "d"], ctx=use), ["c", "d"], "cpu")
    return run


def _raised(rec, label, fn, *args, **kwargs):
    """The call under its label -> what it raised: the class, index and name where the exception has them, the text; or "no error"."""
    try:
        rec.call(label, fn, *args, **kwargs)
        return "no error"
    except Exception as e:  # noqa: BLE001 (the class is what is recorded)
        return {"error": type(e).__name__, "index": getattr(e, "index", None), "name": getattr(e, "name", None), "text": str(e)}


def _near(seed: int, x: np.ndarray) -> np.ndarray:
    """x with one byte in sixteen changed: a base for x, or x against a base."""
    rs = np.random.RandomState(seed)
    y = x.copy()
    if len(y):
        at = rs.choice(len(y), max(len(y) // 16, 1), replace=False)
        y[at] ^= rs.randint(1, 256, len(at)).astype(np.uint8)
    return y


def _changed(x: bytes, at: int) -> bytes:
    return x[:at] + bytes([x[at] ^ 0x55]) + x[at + 1:]


def _stored_and_coded(rec, label, blob, c, unpack):
    """One stored and one coded stream of a container with stored flags, damaged as _damaged does it."""
    sizes = np.diff(c["offsets"].astype(np.int64))
    for what, want in (("stored", True), ("coded", False)):
        k = next((k for k in range(len(sizes)) if sizes[k] > 0 and bool(c["stored"][k]) == want), None)
        rec.note(f"{label} {what} stream", k)
        if k is not None:
            _damaged(rec, f"damaged {label} {what}", blob, c, k, unpack)


def _rcxj_stored(stored, checksum, own, plain_items=False):
    def run(rec, ctx):
        use = None if own else ctx
        if plain_items:  # the stored item container: width 1, an item of few values, random ones, empty ones
            widths, lengths = 1, [0, 1, 17, 300, 0, 64]
            flat = _bytes(61, sum(lengths))
            cuts = np.cumsum([0] + lengths)
            items = [(flat[a:b] // 64 if b - a == 300 else flat[a:b]).tobytes() for a, b in zip(cuts[:-1], cuts[1:])]
        else:
            widths = J_WIDTHS
            items = [_noisy_low_planes(60 + i, w, n).tobytes() for i, (w, n) in enumerate(zip(J_WIDTHS, J_LENGTHS))]
        blob = rec.blob("pack_typed_items", container.pack_typed_items, items, widths=widths, ctx=use, checksum=checksum, stored=stored)
        c = container.parse_typed_items(blob)
        rec.note("version stored", [blob[4], None if c.get("stored") is None else c["stored"].astype(int)])
        for pick in (None, [3, 0, 3], [2]):
            want = items if pick is None else [items[k] for k in pick]
            assert rec.call(f"unpack_typed_items {pick}", container.unpack_typed_items, blob, pick=pick, ctx=use) == want
        assert rec.call("unpack_typed_items verify=False", container.unpack_typed_items, blob, ctx=use, verify=False) == items
        if checksum and c.get("stored") is not None:
            _stored_and_coded(rec, "unpack_typed_items", blob, c, lambda bad: container.unpack_typed_items(bad, ctx=use))
    return run


def _tensors_stored(checksum, own):
    def run(rec, ctx):
        import torch
        use = None if own else ctx
        named = {"a": _sorted_ints(51, 8, 100).view(np.int64), "b": torch.zeros(0, dtype=torch.float16), "c": _bytes(52, 50),
                 "d": np.random.RandomState(53).standard_normal((3, 7)).astype(np.float32)}
        blob = rec.blob("pack_tensors", container.pack_tensors, named, block=64, ctx=use, checksum=checksum, stored=True)
        c = container.parse_typed_items(blob)
        rec.note("version stored", [blob[4], None if c.get("stored") is None else c["stored"].astype(int)])
        got = rec.call("unpack_tensors", container.unpack_tensors, blob, ctx=use)
        assert list(got) == list(named) and all(got[k].numpy().tobytes() == torch.as_tensor(named[k]).numpy().tobytes() for k in named)
        if checksum and c.get("stored") is not None:
            _stored_and_coded(rec, "unpack_tensors", blob, c, lambda bad: container.unpack_tensors(bad, ctx=use))
    return run


def _rcxd(width, op, checksum, stored, base_check, own, tensor=False, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        sb = width * 64
        n = 2 * sb + 3 * width + (width - 1)
        ref = _typed_bytes(70 + width, width, n)
        data = _near(80 + width, ref)
        raw, base = data.tobytes(), ref.tobytes()
        src, given = raw, base
        if tensor:
            import torch
            dtype = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[width]
            src, given = (torch.from_numpy(x[: n - n % width].view(dtype).copy()).cuda() for x in (data, ref))
            raw, base, n = raw[: n - n % width], base[: n - n % width], n - n % width
        blob = rec.blob("pack_delta", container.pack_delta, src, given, width=None if tensor else width, block=64, ctx=use, checksum=checksum, stored=stored,
                        op=op, base_check=base_check)
        c = container.parse_delta(blob)
        inner = c["inner"]
        rec.note("op guard stored", [c["op"], c["base_crcs"], None if inner["stored"] is None else inner["stored"].astype(int)])
        assert rec.call("unpack_delta", container.unpack_delta, blob, given, ctx=use) == raw
        assert rec.call("unpack_delta verify=False", container.unpack_delta, blob, base, ctx=use, verify=False) == raw
        for a, b in ((sb - 1, sb + 1), (2 * sb + 1, n), (0, n)):
            assert rec.call(f"unpack_delta_range {a} {b}", container.unpack_delta_range, blob, base, a, b, ctx=use) == raw[a:b]
        assert rec.call("unpack_delta_range verify=False", container.unpack_delta_range, blob, base, sb - 1, sb + 1, ctx=use, verify=False) == raw[sb - 1: sb + 1]
        wrong = _changed(base, sb + 1)  # one byte of the second superblock
        rec.note("wrong base", _raised(rec, "unpack_delta wrong base", container.unpack_delta, blob, wrong, ctx=use))
        assert rec.call("unpack_delta_range beside the wrong byte", container.unpack_delta_range, blob, wrong, 0, sb, ctx=use) == raw[:sb]
        if damage:
            _damaged(rec, "damaged unpack_delta", blob, inner, width, lambda bad: container.unpack_delta(bad, base, ctx=use))  # the first block of the second superblock
            bad = _damaged(rec, "damaged unpack_delta_range", blob, inner, width, lambda bad: container.unpack_delta_range(bad, base, sb, sb + 1, ctx=use))
            assert rec.call("damaged unpack_delta_range beside it", container.unpack_delta_range, bad, base, 0, sb, ctx=use) == raw[:sb]
    return run


K_OPS = {"auto": ["xor", "auto", None, "auto", "auto"], "list": ["xor", None, None, "sub", "subzz"], "name": "subzz"}
K_PREDICTS = {"None": None, "delta": "delta", "list": [None, "auto", "zigzag", None, None], "auto": "auto"}


def _rcxk(ops, predict, checksum, stored, base_check, own, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        items = [_typed_bytes(40 + i, w, n) for i, (w, n) in enumerate(zip(J_WIDTHS, J_LENGTHS))]
        bases = [_near(90 + i, x).tobytes() for i, x in enumerate(items)]
        bases[3] = _bytes(99, J_LENGTHS[3]).tobytes()  # unrelated: where the op is measured, the rule answers "no base"
        items = [x.tobytes() for x in items]
        if isinstance(ops, list):
            bases = [b if o is not None else None for b, o in zip(bases, ops)]
        each = list(predict) if isinstance(predict, list) else predict
        if isinstance(each, list) and not isinstance(ops, list):
            each = [None] * len(items)  # (every item has an op)
        blob = rec.blob("pack_delta_items", container.pack_delta_items, items, bases, widths=J_WIDTHS, ops=ops, predict=each, ctx=use, checksum=checksum,
                        stored=stored, base_check=base_check)
        c = container.parse_delta_items(blob)
        rec.note("ops guard preds", [c["ops"], c["base_crcs"], c["inner"]["preds"]])
        chosen = rec.call("choose_delta_items", container.choose_delta_items, items, bases, widths=J_WIDTHS, ops=ops, predict=each, ctx=use)
        rec.note("choose_delta_items", chosen)
        again = rec.blob("pack_delta_items as chosen", container.pack_delta_items, items, bases, widths=J_WIDTHS, ops=chosen[0], predict=chosen[1], ctx=use,
                         checksum=checksum, stored=stored, base_check=base_check)
        assert again == blob
        for pick in (None, [3, 0, 3], [2]):
            want = items if pick is None else [items[k] for k in pick]
            assert rec.call(f"unpack_delta_items {pick}", container.unpack_delta_items, blob, bases, pick=pick, ctx=use) == want
        assert rec.call("unpack_delta_items verify=False", container.unpack_delta_items, blob, bases, ctx=use, verify=False) == items
        victim = next(k for k in range(len(items)) if c["ops"][k] != container.BASE_OP_NONE and len(items[k]))
        wrong = list(bases)
        wrong[victim] = _changed(bases[victim], len(bases[victim]) // 2)
        rec.note("wrong base", [victim, _raised(rec, "unpack_delta_items wrong base", container.unpack_delta_items, blob, wrong, pick=[4, victim], ctx=use)])
        wrong[victim] = None
        others = [k for k in range(len(items)) if k != victim]
        assert rec.call("unpack_delta_items beside the wrong base", container.unpack_delta_items, blob, wrong, pick=others, ctx=use) == [items[k] for k in others]
        if damage:
            first = int(c["inner"]["sub_first"][3])
            bad = _damaged(rec, "damaged unpack_delta_items", blob, c["inner"], first, lambda bad: container.unpack_delta_items(bad, bases, ctx=use))
            assert rec.call("damaged unpack_delta_items beside it", container.unpack_delta_items, bad, bases, pick=[1, 4], ctx=use) == [items[1], items[4]]
    return run


def _tensors_delta(op, predict, checksum, stored, base_check, own, on_gpu=False, damage=False):
    def run(rec, ctx):
        import torch
        use = None if own else ctx
        named = {"a": _sorted_ints(51, 8, 100).view(np.int64), "b": torch.zeros(0, dtype=torch.float16), "c": _bytes(52, 50),
                 "d": np.random.RandomState(53).standard_normal((3, 7)).astype(np.float32)}
        # the base lacks "b" and has "d" with another shape: only "a" and "c" can lean on it
        base = {"a": _near(54, named["a"].view(np.uint8)).view(np.int64), "c": _near(55, named["c"]), "d": np.zeros((7, 3), np.float32)}
        given, theirs = named, base
        if on_gpu:
            given, theirs = ({k: torch.as_tensor(v).cuda() for k, v in d.items()} for d in (named, base))
        blob = rec.blob("pack_tensors_delta", container.pack_tensors_delta, given, theirs, block=64, op=op, predict=predict, ctx=use, checksum=checksum,
                        stored=stored, base_check=base_check)
        c = container.parse_delta_items(blob)
        rec.note("directory ops guard preds", [c["inner"]["directory"], c["ops"], c["base_crcs"], c["inner"]["preds"]])
        chosen = rec.call("choose_tensors_delta", container.choose_tensors_delta, given, theirs, block=64, op=op, predict=predict, ctx=use)
        rec.note("choose_tensors_delta", chosen)
        again = rec.blob("pack_tensors_delta as chosen", container.pack_tensors_delta, given, theirs, block=64, op=chosen[0], predict=chosen[1], ctx=use,
                         checksum=checksum, stored=stored, base_check=base_check)
        assert again == blob

        def same(got, names, device):
            assert list(got) == names
            for k in names:
                want = torch.as_tensor(named[k])
                assert got[k].device.type == device and got[k].dtype == want.dtype and got[k].shape == want.shape
                assert got[k].cpu().numpy().tobytes() == want.numpy().tobytes()

        same(rec.call("unpack_tensors_delta", container.unpack_tensors_delta, blob, theirs, ctx=use), ["a", "b", "c", "d"], "cpu")
        same(rec.call("unpack_tensors_delta d a", container.unpack_tensors_delta, blob, base, names=["d", "a"], ctx=use), ["d", "a"], "cpu")
        same(rec.call("unpack_tensors_delta cuda", container.unpack_tensors_delta, blob, base, device="cuda", ctx=use), ["a", "b", "c", "d"], "cuda")
        same(rec.call("unpack_tensors_delta verify=False", container.unpack_tensors_delta, blob, base, ctx=use, verify=False), ["a", "b", "c", "d"], "cpu")
        entries = container.parse_tensor_directory(c["inner"]["directory"], c["nitems"])
        leaning = [e["name"] for e in entries if any(c["ops"][k] != container.BASE_OP_NONE for k in range(e["first"], e["first"] + e["count"]))]
        rec.note("leaning", leaning)
        if leaning:
            victim = leaning[0]
            without = {k: v for k, v in base.items() if k != victim}
            rec.note("base without the tensor", _raised(rec, "unpack_tensors_delta base without the tensor", container.unpack_tensors_delta, blob, without, ctx=use))
            same(rec.call("unpack_tensors_delta beside the missing base", container.unpack_tensors_delta, blob, without, names=["d", "b"], ctx=use), ["d", "b"], "cpu")
            flat = base[victim].view(np.uint8).copy()
            flat[len(flat) - 3] ^= 0x55  # (in the tensor's last item)
            wrong = dict(base, **{victim: flat.view(base[victim].dtype).reshape(base[victim].shape)})
            rec.note("wrong base", _raised(rec, "unpack_tensors_delta wrong base", container.unpack_tensors_delta, blob, wrong, ctx=use))
        if damage:
            # "a" is items 0 and 1 of 8 planes each, "c" item 2 of one, "d" item 3: its top plane
            bad = _damaged(rec, "damaged unpack_tensors_delta", blob, c["inner"], 17 + 3, lambda bad: container.unpack_tensors_delta(bad, base, ctx=use))
            same(rec.call("damaged unpack_tensors_delta beside it", container.unpack_tensors_delta, bad, base, names=["c", "a"], ctx=use), ["c", "a"], "cpu")
    return run


PAST = -(1 << 63)  # what table entries at or past the count hold
PICKS = (3, 3, 1)  # the picks of the opened containers' one decode_into: one repeats; behind them comes an entry that names no item


def _tables(nitems, lengths):
    """The device tables of one decode_into: max_pick 8, count 4 -- PICKS back to back and an entry that names no item behind them."""
    import torch
    pick, at = np.full(8, PAST, np.int64), np.full(8, PAST, np.int64)
    pick[:4] = list(PICKS) + [nitems + 2]
    at[:4] = np.concatenate([[0], np.cumsum([lengths[k] for k in PICKS])])
    size = int(at[3]) + 16
    return torch.from_numpy(pick).cuda(), torch.from_numpy(at).cuda(), torch.tensor([4], dtype=torch.int64).cuda(), torch.zeros(size, dtype=torch.uint8).cuda()


def _opened(rec, tag, use, open_, blob, items, typed):
    """Open, reserve, one decode_into, the latch, the buffer's hash, verify, close -> what verify raised, or None."""
    lengths = [len(x) for x in items]
    box = rec.call(f"{tag}open", open_, blob, ctx=use)
    try:
        d_pick, d_at, d_count, d_dst = _tables(len(items), lengths)
        if typed:
            rec.call(f"{tag}reserve", box.reserve, 8, sum(lengths[k] for k in PICKS) + 16)  # (room for the byte of the entry that names no item)
        else:
            rec.call(f"{tag}reserve", box.reserve, 8)
        rec.call(f"{tag}decode_into", box.decode_into, d_pick, d_at, d_count, d_dst, 8)
        st = rec.call(f"{tag}sync_status", box.ctx.sync_status, raise_on_error=False)
        got = d_dst.cpu().numpy()
        latched = [list(st), box.pick_of(st[1])] if typed else list(st)
        result = [latched, hashlib.sha256(got.tobytes()).hexdigest()]
        try:
            if typed:
                rec.call(f"{tag}verify", box.verify, list(PICKS))
            else:
                rec.call(f"{tag}verify", box.verify, d_dst, list(PICKS))
        except container.ChecksumError as e:
            return result, got, {"error": type(e).__name__, "kind": e.kind, "index": e.index, "text": str(e)}
        return result, got, None
    finally:
        rec.call(f"{tag}close", box.close)


def _open(made, own, typed=False, damage=False):
    def run(rec, ctx):
        use = None if own else ctx
        if typed:
            items = [_typed_bytes(40 + i, w, n).tobytes() for i, (w, n) in enumerate(zip(J_WIDTHS, J_LENGTHS))]
            if made == "stored":
                items = [_noisy_low_planes(60 + i, w, n).tobytes() for i, (w, n) in enumerate(zip(J_WIDTHS, J_LENGTHS))]
            blob = rec.blob("pack", container.pack_typed_items, items, widths=J_WIDTHS, predict=None if made == "stored" else [None, "delta", None, "zigzag", "delta"],
                            ctx=ctx, checksum=made == "checked", stored=True if made == "stored" else None)
            open_, c = container.open_typed_items, container.parse_typed_items(blob)
        else:
            flat = _bytes(31, 382) // 3
            items = [flat[a:b].tobytes() for a, b in zip(np.cumsum([0, 0, 1, 17, 300, 0]), np.cumsum([0, 1, 17, 300, 0, 64]))]
            if made == "stored":
                blob = rec.blob("pack", container.pack_typed_items, items, widths=1, stored=True, ctx=ctx)
                c = container.parse_typed_items(blob)
            else:
                blob = rec.blob("pack", container.pack_items, items, ctx=ctx, checksum=made == "checked")
                c = container.parse_items(blob)
            open_ = container.open_items
        result, got, raised = _opened(rec, "", use, open_, blob, items, typed)
        rec.note("latched and sha256", result)
        assert raised is None and got[: sum(len(items[k]) for k in PICKS)].tobytes() == b"".join(items[k] for k in PICKS)
        if damage:  # as _damaged: one bit of item 3's first stream, until verify() raises ChecksumError
            stream = int(c["sub_first"][3]) if typed else 3
            base, lo, hi = len(blob) - len(c["payload"]), int(c["offsets"][stream]), int(c["offsets"][stream + 1])
            assert hi > lo
            places = [hi - 1 - k for k in range(10)] + [(lo + hi) // 2, lo + (hi - lo) // 4, lo + 3 * (hi - lo) // 4] + [lo + 6 + k for k in range(3)]
            tries = []
            for at in dict.fromkeys(p for p in places if lo <= p < hi):
                bad = blob[:base + at] + bytes([blob[base + at] ^ 0x10]) + blob[base + at + 1:]
                result, _, raised = _opened(rec, f"flip {at - lo} ", use, open_, bad, items, typed)
                tries.append([at - lo, raised if raised is not None else {"error": "none from verify"}, result[0]])
                if raised is not None:
                    break
            rec.note("damaged verify", tries)
    return run


def gpu_cases():
    """name -> run(rec, ctx).  The first case of every kind lets the call make and close its own context."""
    cases = {}
    noise = _bytes(11, 197) // 2  # (compressible, so that no block wants storing without being asked)
    half = np.concatenate([np.zeros(128, np.uint8), _bytes(12, 69)])  # two blocks that shrink, two that cannot
    for n in (1, 64, 197):
        for checksum in (False, True):
            cases[f"RCXB n={n} crc={int(checksum)}"] = _rcxb(noise[:n], 64, 0, checksum, None, False, n == 1, RANGES if n == 197 else ())
    for coder in (1, 2, 3):
        for checksum in (False, True):
            cases[f"RCXB coder={coder} crc={int(checksum)}"] = _rcxb(noise, 64, coder, checksum, None, False, False, RANGES)
    for stored in (None, True, 0.25):
        for checksum in (False, True):
            cases[f"RCXB stored={stored} crc={int(checksum)}"] = _rcxb(half, 64, 0, checksum, stored, False, stored is True, RANGES,
                                                                       damage=checksum and stored is not None)
    for checksum in (False, True):
        cases[f"RCXB blksort crc={int(checksum)}"] = _rcxb(_bytes(13, 32768 + 300) // 16, 4096, 0, checksum, None, True, not checksum, ())
    cases["RCXB damaged"] = _rcxb(noise, 64, 0, True, None, False, False, (), damage=True)
    for checksum in (False, True):
        cases[f"RCXI crc={int(checksum)}"] = _rcxi(checksum, not checksum, damage=checksum)
    for width in (2, 4, 8):
        n = 2 * width * 64 + 3 * width + (width - 1)
        for predict in (None, "delta", "zigzag", "auto"):
            for checksum in (False, True):
                cases[f"RCXT width={width} predict={predict} crc={int(checksum)}"] = _rcxt(_typed_bytes(20 + width, width, n), width, predict, checksum, None,
                                                                                          width == 2 and predict is None, damage=checksum and predict == "delta")
        for checksum in (False, True):
            cases[f"RCXT width={width} stored crc={int(checksum)}"] = _rcxt(_noisy_low_planes(30 + width, width, n), width, None, checksum, True, False, damage=checksum)
        cases[f"RCXT width={width} stored=0.25 auto"] = _rcxt(_typed_bytes(20 + width, width, n), width, "auto", True, 0.25, False)
    cases["RCXT a GPU tensor"] = _rcxt(_typed_bytes(24, 4, 2 * 4 * 64 + 12), 4, "auto", True, None, True, tensor=True)
    for predict in (None, [None, "delta", None, "zigzag", "delta"], "auto"):
        tag = "list" if isinstance(predict, list) else predict
        for checksum in (False, True):
            cases[f"RCXJ predict={tag} crc={int(checksum)}"] = _rcxj(predict, checksum, b"", predict is None, damage=checksum and predict is None)
    cases["RCXJ directory"] = _rcxj("auto", True, b"a directory", False)
    for predict in (None, {"a": "delta", "d": "auto", "c": "zigzag"}):
        for checksum in (False, True):
            cases[f"tensors predict={'dict' if predict else None} crc={int(checksum)}"] = _tensors(predict, checksum, predict is None,
                                                                                                   damage=checksum and predict is not None)
    cases["tensors on the GPU"] = _tensors("auto", True, False, on_gpu=True)
    # stored sub-items: RCXJ version 2, the stored item container, tensors
    cases["RCXJ stored=True crc=0"] = _rcxj_stored(True, False, True)
    cases["RCXJ stored=0.25 crc=1"] = _rcxj_stored(0.25, True, False)
    cases["RCXJ width 1 stored=True crc=1"] = _rcxj_stored(True, True, False, plain_items=True)
    cases["RCXJ width 1 stored=0.25 crc=0"] = _rcxj_stored(0.25, False, False, plain_items=True)
    cases["tensors stored"] = _tensors_stored(True, False)
    # RCXD: every width and every op once; checksum, stored and base_check each both ways
    for i, (width, op, checksum, stored, base_check) in enumerate(((1, "xor", False, None, True), (2, "sub", True, True, False), (4, "subzz", True, 0.25, True),
                                                                   (8, "auto", False, True, True), (1, "auto", True, None, False))):
        cases[f"RCXD width={width} op={op} crc={int(checksum)} stored={stored} guard={int(base_check)}"] = _rcxd(width, op, checksum, stored, base_check, i == 0,
                                                                                                              damage=checksum and i >= 2)
    cases["RCXD GPU tensors"] = _rcxd(4, "auto", True, None, True, False, tensor=True)
    # RCXK: every form of ops and every form of predict
    for i, (otag, ptag, checksum, stored, base_check) in enumerate((("auto", "None", False, None, True), ("auto", "list", True, 0.25, True), ("auto", "auto", False, True, True),
                                                                    ("list", "delta", True, None, False), ("name", "auto", True, 0.25, True))):
        cases[f"RCXK ops={otag} predict={ptag} crc={int(checksum)} stored={stored} guard={int(base_check)}"] = _rcxk(K_OPS[otag], K_PREDICTS[ptag], checksum, stored,
                                                                                                                 base_check, i == 0, damage=i == 1)
    # tensors against a base
    for i, (otag, op, predict, checksum, stored, base_check) in enumerate((("subzz", "subzz", None, False, None, True),
                                                                           ("dict", {"a": "xor", "c": None}, {"d": "auto", "c": "delta"}, False, True, False),
                                                                           ("auto", "auto", {"d": "auto", "c": "delta"}, True, True, True))):
        cases[f"tensors-delta op={otag} predict={'dict' if predict else None} crc={int(checksum)} stored={stored} guard={int(base_check)}"] = _tensors_delta(
            op, predict, checksum, stored, base_check, i == 0, damage=i == 2)
    cases["tensors-delta on the GPU"] = _tensors_delta("auto", "auto", True, None, True, False, on_gpu=True)
    # the opened containers: an owned and a given context each
    for made in ("plain", "stored", "checked"):
        cases[f"open_items {made}"] = _open(made, made == "plain", damage=made == "checked")
        cases[f"open_typed_items {made}"] = _open(made, made == "plain", typed=True, damage=made == "checked")
    return cases


def run_gpu_case(run, ctx, setattr_=None):
    """One case under a Recorder -> its record.  setattr_: a test's monkeypatch.setattr; None: recording() puts and removes the wrappers."""
    if setattr_ is None:
        with recording() as rec:
            run(rec, ctx)
    else:
        rec = Recorder()
        rec.install(setattr_)
        run(rec, ctx)
    return rec.record
