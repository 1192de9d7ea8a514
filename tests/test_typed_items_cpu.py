"""The typed stage per item as far as it goes without a GPU: the header against typed_items.EXPORTS and the built library,
the sub-item table against numpy, the numpy restatement (typed_items.split_numpy / join_numpy) against predict_cases on
common ground, the RCXJ layout byte for byte with every refusal of parse_typed_items, the JSON directory, the per-item rule
of predict="auto" on the buffers it is for, the sizes the documents quote from the CPU oracle, and the plan and mapping of
csrc/rcx_typed_items.hpp in a sanitized program over the whole case list."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import planes_cases as pc
import predict_cases as pr
import stats_cases as sc
import typed_items_cases as tc
from cpprcoder_amd import container, stats, typed_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_typed_items.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, rcx
    build.build()
    names = declared_symbols()
    assert len(names) == 6 and set(names) == set(typed_items.EXPORTS), (names, typed_items.EXPORTS)
    for name in names:
        assert getattr(typed_items.lib(), name).argtypes is not None
    assert '#include "rcx_predict.h"' in open(os.path.join(ROOT, "include", "rcx_typed_items.h")).read()
    # rcx.h and the other headers are what they were
    assert len(rcx.EXPORTS) == 57 and len(planes.EXPORTS) == 4 and len(predict.EXPORTS) == 4 and len(stats.EXPORTS) == 4 and rcx.lib().rcx_version() == 300
    assert not set(typed_items.EXPORTS) & (set(rcx.EXPORTS) | set(planes.EXPORTS) | set(predict.EXPORTS) | set(stats.EXPORTS))
    assert all(h in build.HEADERS for h in ("rcx_typed_items.hpp", "rcx_typed_items_api.hpp")) and any(h.endswith("rcx_typed_items.h") for h in build.HEADERS)
    assert (typed_items.NONE, typed_items.DELTA, typed_items.ZIGZAG) == (0, 1, 2) and typed_items.WIDTHS == (1, 2, 4, 8)


def test_sub_offsets_against_numpy():
    for case in tc.kernel_cases():
        for base in (0, 77):
            offs = tc.offsets_of(case, base)
            want = typed_items.sub_offsets_numpy(offs, case["widths"])
            assert len(want) == int(case["widths"].astype(np.int64).sum()) + 1 == typed_items.sub_count(case["widths"]) + 1
            assert np.array_equal(typed_items.sub_offsets(offs, case["widths"]), want), case["name"]
            assert int(want[0]) == base and int(want[-1]) == int(offs[-1])
    # by hand: 23 bytes of width 4 are five elements and three tail bytes; width 1 is one sub-item; an empty item has empty ones
    assert list(typed_items.sub_offsets([10, 33, 33, 40, 51], [4, 2, 1, 8])) == [10, 15, 20, 25, 33, 33, 33, 40, 41, 42, 43, 44, 45, 46, 47, 51]
    assert list(typed_items.sub_offsets_numpy([10, 33, 33, 40, 51], [4, 2, 1, 8])) == [10, 15, 20, 25, 33, 33, 33, 40, 41, 42, 43, 44, 45, 46, 47, 51]
    assert typed_items.sub_count([]) == 0 and list(typed_items.sub_offsets([5], [])) == [5]
    # what the C calls refuse without a GPU
    L = typed_items.lib()
    out = np.zeros(16, np.uint64)
    for offs, widths in (([0, 8], [3]), ([0, 8], [0]), ([0, 8], [16]), ([8, 0], [2]), ([0, 8 * ((1 << 24) - 255)], [8]), ([0, (1 << 24) - 255], [1]),
                         ([0, (1 << 24) - 256 + 1], [2])):
        o, w = np.array(offs, np.uint64), np.array(widths, np.uint8)
        if offs == [0, (1 << 24) - 256 + 1] and widths == [2]:
            assert L.rcx_typed_items_sub_offsets(o.ctypes.data, w.ctypes.data, 1, out.ctypes.data) == 0  # m + r below the limit
            continue
        assert L.rcx_typed_items_sub_offsets(o.ctypes.data, w.ctypes.data, 1, out.ctypes.data) == -2, (offs, widths)
    assert typed_items.sub_count([2, 3]) == 0 and L.rcx_typed_items_sub_offsets(None, None, 1, out.ctypes.data) == -2
    assert L.rcx_typed_items_sub_offsets(None, None, 0, None) == -2 and L.rcx_typed_items_sub_offsets(None, None, 0, out.ctypes.data) == 0


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_worked_vector_and_the_item_borders():
    x = np.frombuffer(bytes.fromhex("0100030006 00FFFF0200AA".replace(" ", "")), np.uint8)
    assert typed_items.split_numpy(x, [0, 11], [2], [1]).tobytes() == bytes.fromhex("0102 03F9 0300 0000 FF00 AA".replace(" ", ""))
    assert typed_items.split_numpy(x, [0, 11], [2], [2]).tobytes() == bytes.fromhex("0204 060D 0600 0000 0000 AA".replace(" ", ""))
    assert typed_items.split_numpy(x, [0, 11], [1]).tobytes() == x.tobytes()
    # two items of one buffer: the predictor starts again, each item's planes stay in its span, bytes outside stay
    e = np.array([10, 11, 13, 1000, 1001, 999], "<u4").view(np.uint8)
    y = typed_items.split_numpy(np.concatenate([[0xEE], e, [0xDD]]).astype(np.uint8), [1, 13, 25], [4, 4], [1, 1])
    assert y[0] == 0xEE and y[25] == 0xDD
    assert y[1:13].tobytes() == bytes([10, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]) and y[13:25].tobytes() == bytes([0xE8, 1, 0xFE, 3, 0, 0xFF, 0, 0, 0xFF, 0, 0, 0xFF])
    for bad in (([0, 4], [3], None), ([0, 4], [1], [1]), ([0, 4], [2], [3]), ([4, 0], [2], None), ([0, 40], [2], None)):
        with pytest.raises(ValueError):
            typed_items.split_numpy(np.zeros(8, np.uint8), *bad)


@pytest.mark.parametrize("width", pr.WIDTHS)
def test_superblock_cut_items_are_the_existing_transform(width):
    rs = np.random.RandomState(width)
    for block, n in ((16, 5 * width * 16 + width + 1), (100, 3 * width * 100 + 37), (4096, 3 * width * 4096 + 37), (48, 48 * width), (100, width - 1)):
        x = rs.randint(0, 256, n, dtype=np.uint8)
        for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG):
            lengths, widths, preds = tc.superblock_items(n, width, block, pred)
            offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
            y = typed_items.split_numpy(x, offs, widths, preds)
            assert np.array_equal(y, pr.split_numpy(x, width, block, pred)), (width, block, n, pred)
            assert np.array_equal(typed_items.join_numpy(y, offs, widths, preds), x)
            # and its sub-items are the coder's blocks: all whole ones but those of the ragged rest
            sub = np.diff(typed_items.sub_offsets_numpy(offs, widths).astype(np.int64))
            assert bool((sub[: (n // (width * block)) * width] == block).all()) and int(sub.sum()) == n


def test_numpy_restatement_over_the_case_list():
    noise = np.random.RandomState(9).randint(0, 256, 4 << 20, dtype=np.uint8)
    cases = tc.kernel_cases()
    assert len(cases) == 25 and {(c["src_offset"], c["dst_offset"]) for c in cases} == {(a, b) for a in tc.OFFSETS for b in tc.OFFSETS}
    seen = set()
    for k, case in enumerate(cases):
        seen |= {(int(w), int(p)) for w, p in zip(case["widths"], case["preds"])}
        for kind in tc.KINDS if k % 4 == 0 else ("random",):
            x = tc.case_bytes(case, kind, noise[k:])
            offs = tc.offsets_of(case)
            y = typed_items.split_numpy(x, offs, case["widths"], case["preds"])
            assert np.array_equal(y, tc.split_expected(case, x)), (case["name"], kind)
            assert np.array_equal(typed_items.join_numpy(y, offs, case["widths"], case["preds"]), x), (case["name"], kind)
            assert np.array_equal(tc.join_expected(case, y), x)
    assert seen == {(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)}
    for w in tc.WIDTHS:  # the switch points are in the list
        step = 16 // w * 256 * 16
        for n in (0, 1, w, 16 * w - 1, 16 * w + 1, 17 * 16 * w, 1023 * w, 1025 * w, 4095 * w, 4097 * w, (step - 1) * w, (step + 1) * w, 2053 * w):
            assert n in tc.switch_lengths(w), (w, n)


# ---- the mapping, sanitized ------------------------------------------------------------------------------------------------------
def test_plan_and_mapping_in_a_sanitized_program(tmp_path):
    """tests/sim/typed_items_san.cpp: rcx_typed_plan and the functions that map a step, a row, a lane and a rest lane to an item's
    bytes, in a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer.  Over the whole case list, split and
    join, with grids that loop: every byte of every item is read once and written once, nothing else is touched."""
    exe, cases = str(tmp_path / "typed_items_san"), str(tmp_path / "cases.txt")
    tc.write_cases(cases, tc.kernel_cases())
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "typed_items_san.cpp")], check=True)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "typed_items_san ok: 25 batches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- RCXJ ------------------------------------------------------------------------------------------------------------------------
LENGTHS, WIDTHS, PREDS = [23, 0, 7, 16], [4, 2, 1, 8], [2, 0, 0, 1]   # sub-items: 5 5 5 8 | 0 0 | 7 | 2 2 2 2 2 2 2 2
SUB = [5, 5, 5, 8, 0, 0, 7] + [2] * 8
SIZES = [9, 9, 9, 12, 0, 0, 11] + [6] * 8
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
PAYLOAD = bytes(range(int(OFFS[-1])))


def blob_j(crcs=None, directory=b"", coder=1, lengths=LENGTHS, widths=WIDTHS, preds=PREDS, offs=OFFS, payload=PAYLOAD):
    return container.typed_items_header_bytes(coder, lengths, widths, preds, offs, crcs, directory) + payload


def test_layout_byte_for_byte():
    crcs = np.arange(100, 115, dtype=np.uint32)
    fixed = struct.pack("<4sBBHQQQ", b"RCXJ", 1, 1, 0, 4, 15, 0)
    tables = struct.pack("<4Q", *LENGTHS) + bytes(WIDTHS) + bytes(PREDS) + OFFS.astype("<u8").tobytes()
    assert len(fixed) == 32 and blob_j() == fixed + tables + PAYLOAD
    fixed = struct.pack("<4sBBHQQQ", b"RCXJ", 1, 1, 2, 4, 15, 5)
    assert blob_j(crcs, b"hello") == fixed + tables + crcs.astype("<u4").tobytes() + b"hello" + PAYLOAD
    c = container.parse_typed_items(blob_j(crcs, b"hello"))
    assert (c["coder"], c["flags"], c["nitems"], c["nsub"], c["directory"]) == (1, 2, 4, 15, b"hello")
    assert list(c["lengths"]) == LENGTHS and list(c["widths"]) == WIDTHS and list(c["preds"]) == PREDS and list(c["sub_lengths"]) == SUB
    assert list(c["sub_first"]) == [0, 4, 6, 7, 15] and np.array_equal(c["offsets"], OFFS) and np.array_equal(c["crcs"], crcs)
    assert bytes(c["payload"]) == PAYLOAD and container.parse_typed_items(blob_j())["crcs"] is None
    # nothing at all
    empty = container.typed_items_header_bytes(0, [], [], None, [0])
    assert empty == struct.pack("<4sBBHQQQ", b"RCXJ", 1, 0, 0, 0, 0, 0) + bytes(8) and container.parse_typed_items(empty)["nitems"] == 0
    assert container.unpack_typed_items(empty) == [] and container.pack_typed_items([]) == empty


def test_refusals():
    def with_bytes(b, at, value):
        out = bytearray(b)
        out[at: at + len(value)] = value
        return bytes(out)

    good, checked = blob_j(), blob_j(np.zeros(15, np.uint32), b"dir")
    t = 32  # where the tables begin
    bad = [with_bytes(good, 0, b"RCXI"), with_bytes(good, 4, b"\x02"), with_bytes(good, 4, b"\x00"), with_bytes(good, 5, b"\x04"),   # magic, version, coder
           with_bytes(good, 6, b"\x01"), with_bytes(good, 6, b"\x04"), with_bytes(good, 7, b"\x01"), with_bytes(good, 6, b"\x02"),   # flags (bit 1 without a table)
           with_bytes(good, t + 32, b"\x03"), with_bytes(good, t + 32, b"\x00"), with_bytes(good, t + 33, b"\x10"),                  # widths
           with_bytes(good, t + 36, b"\x03"), with_bytes(good, t + 38, b"\x01"), with_bytes(good, t + 38, b"\x02"),                  # predictors; one on width 1
           with_bytes(good, 16, struct.pack("<Q", 14)), with_bytes(good, 16, struct.pack("<Q", 16)),                                 # nsub is the sum of the widths
           with_bytes(good, 8, struct.pack("<Q", 5)), with_bytes(good, 8, struct.pack("<Q", 1 << 60)),                               # nitems
           with_bytes(good, 24, struct.pack("<Q", 1)), with_bytes(good, 24, struct.pack("<Q", 1 << 62)),                             # the directory's length
           with_bytes(good, t, struct.pack("<Q", 8 * (1 << 24))),                                                                   # a sub-item above the coder's limit
           good + b"x", good[:-1], good[: t + 40], good[:31], checked[:-1], checked[: t + 40 + 8 * 16 + 59],                           # truncated
           with_bytes(good, t + 40, struct.pack("<Q", 1)),                                                                          # offsets[0]
           with_bytes(good, t + 40 + 8, struct.pack("<Q", 40)),                                                                     # decreasing
           with_bytes(good, t + 40 + 8 * 5, struct.pack("<Q", 40)),                                                                 # an empty sub-item with a stream
           with_bytes(good, t + 40 + 8 * 8, OFFS.astype("<u8")[7:8].tobytes())]                                                    # a sub-item with bytes and none
    for k, damaged in enumerate(bad):
        with pytest.raises(container.ContainerError):
            container.parse_typed_items(damaged)
            print("not refused:", k)
    assert container.parse_typed_items(checked)["directory"] == b"dir"
    for parse in (container.parse, container.parse_items, container.parse_typed):  # the other containers do not read it
        with pytest.raises(container.ContainerError):
            parse(good)
    for other in (container.header_bytes(0, 4096, 0, [0]), container.item_header_bytes(0, [], [0]), container.typed_header_bytes(0, 4096, 0, 4, [0])):
        with pytest.raises(container.ContainerError):
            container.parse_typed_items(other)
    # what the header function refuses
    for kw in (dict(widths=[4, 2, 1, 3]), dict(preds=[2, 0, 1, 1]), dict(preds=[3, 0, 0, 1]), dict(widths=[4, 2, 1]), dict(offs=OFFS[:-1]),
               dict(crcs=np.zeros(14, np.uint32)), dict(lengths=[23, 0, 7, 8 * (1 << 24)])):
        with pytest.raises(container.ContainerError):
            blob_j(**kw)


def test_what_pack_typed_items_refuses_before_it_needs_a_gpu():
    ints = np.arange(64, dtype=np.int64)
    for kw in (dict(predict="xor"), dict(predict=1), dict(predict=["delta", "delta"]), dict(predict=[b"delta"]), dict(widths=3), dict(widths=[8, 8]),
               dict(widths=[16]), dict(widths=[1], predict=["delta"]), dict(widths=True)):
        with pytest.raises(container.ContainerError):
            container.pack_typed_items([ints], **kw)
    with pytest.raises(container.ContainerError):
        container.pack_typed_items([b"abcdefgh"])  # plain bytes need a width
    with pytest.raises(container.ContainerError):
        container.pack_typed_items([np.zeros(4, np.complex128)])
    # nothing to code: a header and no GPU, whatever is asked for
    blob = container.pack_typed_items([b"", np.zeros(0, np.int32), np.zeros(0, np.uint8)], widths=[2, 4, 1], predict=["auto", "zigzag", None], checksum=True,
                                      directory=b"d")
    c = container.parse_typed_items(blob)
    assert (c["nitems"], c["nsub"], list(c["widths"]), list(c["preds"]), list(c["crcs"]), c["directory"]) == (3, 7, [2, 4, 1], [0, 2, 0], [0] * 7, b"d")
    assert container.unpack_typed_items(blob) == [b"", b"", b""] and container.unpack_typed_items(blob, pick=[2, 2]) == [b"", b""]
    assert container.unpack_typed_items(blob, pick=[]) == []
    for pick in ([3], [-1]):
        with pytest.raises(container.ContainerError):
            container.unpack_typed_items(blob, pick=pick)


# ---- tensors with names --------------------------------------------------------------------------------------------------------
def test_directory_round_trip_and_empty_tensors_need_no_gpu():
    entries = [{"name": "w", "dtype": "bfloat16", "shape": (3, 4), "first": 0, "count": 2}, {"name": "norm.ä", "dtype": "float32", "shape": (), "first": 2, "count": 1},
               {"name": "none", "dtype": "int64", "shape": (0, 7), "first": 3, "count": 0}]
    raw = container.tensor_directory_bytes(entries)
    assert json.loads(raw.decode())[1] == {"name": "norm.ä", "dtype": "float32", "shape": [], "first": 2, "count": 1}
    assert container.parse_tensor_directory(raw, 3) == entries
    for bad, nitems in ((raw, 2), (b"{}", 3), (b"\xff", 3), (b"[{\"name\":\"a\"}]", 3), (container.tensor_directory_bytes([entries[0], entries[0]]), 3),
                        (container.tensor_directory_bytes([dict(entries[0], first=-1)]), 3)):
        with pytest.raises(container.ContainerError):
            container.parse_tensor_directory(bad, nitems)
    torch = pytest.importorskip("torch")
    named = {"a": torch.zeros(0, 5, dtype=torch.bfloat16), "b": np.zeros((2, 0), np.int64), "c": torch.zeros(0, dtype=torch.bool)}
    blob = container.pack_tensors(named, predict="auto", checksum=True)
    c = container.parse_typed_items(blob)
    assert c["nitems"] == 0 and [e["dtype"] for e in container.parse_tensor_directory(c["directory"], 0)] == ["bfloat16", "int64", "bool"]
    back = container.unpack_tensors(blob)
    assert list(back) == ["a", "b", "c"] and [tuple(t.shape) for t in back.values()] == [(0, 5), (2, 0), (0,)]
    assert [t.dtype for t in back.values()] == [torch.bfloat16, torch.int64, torch.bool]
    assert list(container.unpack_tensors(blob, names=["c"])) == ["c"]
    with pytest.raises(container.ContainerError):
        container.unpack_tensors(blob, names=["d"])
    with pytest.raises(container.ContainerError):
        container.pack_tensors({"z": torch.zeros(4, dtype=torch.complex128)})
    with pytest.raises(container.ContainerError):
        container.pack_tensors({"z": torch.zeros(4, 4)[:, 1]})
    with pytest.raises(container.ContainerError):
        container.unpack_tensors(container.pack_typed_items([], directory=b"not json"))


# ---- the rule, per item --------------------------------------------------------------------------------------------------------
BUFFERS = ("bf16", "fp32", "sorted_keys", "indices")  # 1 MiB each: the state dict of the documents
BLOCK = 65536


@pytest.fixture(scope="module")
def four():
    """name -> (bytes, width, lengths of its superblock items)"""
    out = {}
    for name in BUFFERS:
        x, width = sc.typed_bytes(name)
        out[name] = (x, width, tc.superblock_items(len(x), width, BLOCK, 0)[0])
    return out


def item_costs(x, lengths, width):
    """[nitems, 3]: the summed sub-item costs of every item under none, delta and zigzag, from stats.cost_numpy of split_numpy's output."""
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    widths = np.full(len(lengths), width, np.uint8)
    sub = typed_items.sub_offsets_numpy(offs, widths)
    out = np.zeros((len(lengths), 3), np.uint64)
    for pred in (0, 1, 2):
        y = typed_items.split_numpy(x, offs, widths, np.full(len(lengths), pred, np.uint8))
        cost = stats.cost_numpy(sc.hist_items(y, sub))
        out[:, pred] = cost.reshape(len(lengths), width).sum(axis=1, dtype=np.uint64)
    return out


def test_the_rule_per_item(four):
    picks = {}
    for name, (x, width, lengths) in four.items():
        costs = item_costs(x, lengths, width)
        picks[name] = [container.pick_predictor(*(int(v) for v in row)) for row in costs]
        print(name, [sc.cost_bytes(v) for v in costs.sum(axis=0)], picks[name][:3])
    assert picks["sorted_keys"] == ["delta"] * 2 and picks["indices"] == [None] * 2
    assert picks["bf16"] == [None] * 8 and picks["fp32"] == [None] * 4
    # pinned: the first item of the sorted keys, in bytes to the nearest
    x, width, lengths = four["sorted_keys"]
    assert [sc.cost_bytes(v) for v in item_costs(x, lengths[:1], width)[0]] == PINNED_KEYS_ITEM0


PINNED_KEYS_ITEM0 = [236734, 117499, 117512]  # none, delta, zigzag (the whole MiB: 473449, 234865, 234887)


# ---- the sizes the documents quote ---------------------------------------------------------------------------------------------
def test_sizes_quoted_from_the_oracle(four, oracle):
    """The adaptive coder at 64 KiB blocks: one RCXT of width 8 over the four buffers glued, the four buffer by buffer with
    their own widths -- which is what the sub-items of their superblock-cut typed items are -- and those with delta on the
    sorted keys only; and 1 MiB of int64 indices with planes."""
    glued = np.concatenate([four[name][0] for name in BUFFERS])
    assert pc.total_size(oracle, pc.split_numpy(glued, 8, BLOCK), BLOCK, 0) == 2_310_740
    each, with_delta = {}, {}
    for name, (x, width, lengths) in four.items():
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        widths = np.full(len(lengths), width, np.uint8)
        for table, pred in ((each, 0), (with_delta, 1 if name == "sorted_keys" else 0)):
            y = typed_items.split_numpy(x, offs, widths, np.full(len(lengths), pred, np.uint8))
            assert bool((np.diff(typed_items.sub_offsets_numpy(offs, widths).astype(np.int64)) == BLOCK).all())  # the sub-items are the blocks
            table[name] = pc.total_size(oracle, y, BLOCK, 0)
    print(each, with_delta)
    assert sum(each.values()) == 2_310_749 and sum(with_delta.values()) == 2_072_650
    assert (each["sorted_keys"], with_delta["sorted_keys"]) == (477_361, 239_262) and each["indices"] == 260_084
    assert all(each[name] == with_delta[name] for name in BUFFERS if name != "sorted_keys")
    plain = pc.total_size(oracle, four["indices"][0], BLOCK, 0)
    assert plain == 367_259 and round(100 * (1 - 260_084 / plain)) == 29  # 29 % smaller with planes
