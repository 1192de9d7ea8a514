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


def cpu_section():
    c = container
    sets = header_sets()
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
        "no_gpu": no_gpu_returns(),
    }


# ---- the GPU section: blobs and call traces --------------------------------------------------------------------------------------
DEVICE_CALLS = ("stored.mix_device", "stored.decode_device", "predict.split_device", "predict.join_device", "typed_items.split_device", "typed_items.join_device",
                "stats.blocks_device", "stats.items_device")


def _logged(log, name, fn):
    def call(*args, **kwargs):
        if name != "close" or getattr(args[0], "_h", None):  # (a close that destroys a context: the one from __del__ behind it is none)
            log.append(name)
        return fn(*args, **kwargs)
    return call


class Recorder:
    """Keeps, per labelled public call, the names of the rcx.Context methods and module device calls made inside it, in order.
    install(setattr) puts the recording wrappers in place through the caller's setattr(target, name, value) -- a test's
    monkeypatch.setattr -- which is also what takes them out again."""

    def __init__(self):
        self.log, self.record = [], {"traces": {}}

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

    def call(self, label, fn, *args, **kwargs):
        del self.log[:]
        try:
            return fn(*args, **kwargs)
        finally:
            assert label not in self.record["traces"], label
            self.record["traces"][label] = list(self.log)

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
