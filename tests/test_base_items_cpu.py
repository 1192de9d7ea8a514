"""Residuals against a base per item as far as they go without a GPU: the numpy twin (cpprcoder_amd/base_items.py) pinned by the
worked example of include/rcx_base_items.h and held to base.py and typed_items.py item by item, its inverse over every
batch, the plan and the mapping of csrc/rcx_base_items.hpp in a sanitized program over the whole case list, the header
against base_items.EXPORTS and the built library, the RCXK layout byte for byte with every refusal, what the container calls
refuse before they need a GPU, and with the CPU oracle the sizes the documents quote for a state dict against the one before it."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import base_cases
import base_items_cases as bc
import stored_items_cases as sic
import typed_items_cases as tc
from cpprcoder_amd import base, base_items as bi, container, layout, typed_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = bytes.fromhex("05 01 00 01 42 00 AA 01 00 03 00 06 00 FF FF 02 00 AA")
BASE = bytes.fromhex("EE EE 00 01 02 01 42 00 55")
EXAMPLE = ([0, 7, 18], [2, 1 << 40], [2, 2], [0, 1])  # offsets, base offsets (item 1 has none: anything), widths, predictors


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_worked_example_pins_the_twin():
    text = open(os.path.join(ROOT, "include", "rcx_base_items.h")).read()
    typed = "01 02 03 F9 03 00 00 00 FF 00 AA"
    for op, want in ((bi.XOR, "05 02 00 00 00 00 AA"), (bi.SUB, "05 FE 00 00 FF 00 AA"), (bi.SUBZZ, "0A 03 00 00 00 00 AA")):
        y = bi.split_numpy(SOURCE, BASE, *EXAMPLE, [op, bi.NO_BASE])
        assert y.tobytes() == bytes.fromhex(want + typed), (op, y.tobytes().hex())
        assert bi.join_numpy(y, BASE, *EXAMPLE, [op, bi.NO_BASE]).tobytes() == SOURCE
        assert want in text and want in open(os.path.join(ROOT, "include", "rcx_base.h")).read()
    for piece in ("05 01 00 01 42 00 AA", "01 00 03 00 06 00 FF FF 02 00 AA", "EE EE 00 01 02 01 42 00 55", "0A 03 00 00 00 00 AA   " + typed):
        assert piece in text  # the header's own bytes
    assert typed in open(os.path.join(ROOT, "include", "rcx_typed_items.h")).read()
    assert re.search(r"#define RCX_BASE_NONE 0xFFu\b", text) and bi.NO_BASE == 0xFF == layout.BASE_OP_NONE
    # no table of ops, and a table that says "none" everywhere, are typed_items' transform; no base is looked at
    assert np.array_equal(bi.split_numpy(SOURCE, None, EXAMPLE[0], None, EXAMPLE[2], EXAMPLE[3], None), typed_items.split_numpy(SOURCE, *EXAMPLE[::2], EXAMPLE[3]))
    assert np.array_equal(bi.split_numpy(SOURCE, None, *EXAMPLE, [0xFF, 0xFF]), typed_items.split_numpy(SOURCE, EXAMPLE[0], EXAMPLE[2], EXAMPLE[3]))
    for bad in (lambda: bi.split_numpy(SOURCE, BASE, *EXAMPLE, [3, 0xFF]), lambda: bi.split_numpy(SOURCE, BASE, *EXAMPLE, [0xFF, 1]),   # an op; a predictor AND an op
                lambda: bi.split_numpy(SOURCE, BASE, EXAMPLE[0], [3, 0], EXAMPLE[2], None, [1, 0xFF]),                              # a span past the base
                lambda: bi.split_numpy(SOURCE, BASE, *EXAMPLE, [1]), lambda: bi.split_numpy(SOURCE, BASE, EXAMPLE[0], [2], *EXAMPLE[2:], [1, 0xFF])):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20262).randint(0, 256, (9 << 20) + 64, dtype=np.uint8)


@pytest.fixture(scope="module")
def cases():
    return bc.kernel_cases()


def test_the_case_list_is_what_the_kernels_need(cases):
    names = [c["name"] for c in cases]
    assert len(cases) == 30 and len(set(names)) == 30 and len(bc.ITEM_KINDS) == 22
    for w in bc.WIDTHS:
        step = bc.ROWS[w] * 256 * 16 * w  # bytes of a workgroup step: 32 KiB in every class
        assert step == 32768 and {step - w, step, step + w} <= set(bc.switch_lengths(w))
    mixed = cases[names.index("mixed small")]
    assert len(mixed["lengths"]) == 700 and len(cases[names.index("mixed many")]["lengths"]) == 6000
    assert {(int(w), int(p), int(o)) for w, p, o in zip(mixed["widths"], mixed["preds"], mixed["ops"])} == set(bc.ITEM_KINDS)
    assert not (cases[names.index("none with a base")]["ops"] != bc.NO_BASE).any() and (cases[names.index("all with a base")]["ops"] != bc.NO_BASE).all()
    one = cases[names.index("many on one span")]
    assert one["layout"] == "one" and set(bc.base_layout(one)[0].tolist()) == {0}
    rev = cases[names.index("reverse order")]
    spans = bc.base_layout(rev)[0][rev["ops"] != bc.NO_BASE].astype(np.int64)
    assert rev["layout"] == "reverse" and bool((np.diff(spans) <= 0).all())
    assert {(c["src_offset"], c["base_offset"]) for c in cases} >= {(a, b) for a in (0, 1) for b in (0, 1, 3, 8, 15)}
    assert {c["dst_offset"] for c in cases} == set(bc.OFFSETS)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_the_twin_is_the_existing_twins_item_by_item_and_its_inverse_inverts(cases, noise, kind):
    for k, case in enumerate(cases):
        x, ref = bc.case_data(case, kind, noise[k:])
        offs, (boffs, _) = bc.offsets_of(case).astype(np.int64), bc.base_layout(case)
        tables = (offs, boffs, case["widths"], case["preds"], case["ops"])
        y = bi.split_numpy(x, ref, *tables)
        assert np.array_equal(bi.join_numpy(y, ref, *tables), x), case["name"]
        for i in range(0, len(case["widths"]), 1 if len(case["widths"]) < 100 else 37):  # every item, or a sample of many
            a, b, w, p, op = int(offs[i]), int(offs[i + 1]), int(case["widths"][i]), int(case["preds"][i]), int(case["ops"][i])
            if op == bc.NO_BASE:
                want = typed_items.split_numpy(x[a:b], [0, b - a], [w], [p])
            elif b - a < w:
                want = x[a:b]
            else:
                want = base.split_numpy(x[a:b], ref[int(boffs[i]): int(boffs[i]) + b - a], w, (b - a) // w + 1, op)
            assert np.array_equal(y[a:b], want), (case["name"], i)
    if kind == "equal":  # a residual of nothing but zeros where the source is its base; the tail bytes stay
        case = cases[0]
        x, ref = bc.case_data(case, kind, noise)
        y = bi.split_numpy(x, ref, bc.offsets_of(case), bc.base_layout(case)[0], case["widths"], None, case["ops"])
        assert int(np.count_nonzero(y)) <= int((case["lengths"] % case["widths"].astype(np.uint64)).sum())


@pytest.mark.parametrize("width", bc.WIDTHS)
@pytest.mark.parametrize("op", bc.OPS)
def test_superblock_cut_items_are_the_block_transform(noise, width, op):
    for block in base_cases.BLOCKS:
        n = 3 * width * block + 5
        x, ref = noise[:n], noise[n: 2 * n]
        lengths, widths, ops = bc.superblock_items(n, width, block, op)
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        assert np.array_equal(bi.split_numpy(x, ref, offs, offs[:-1], widths, None, ops), base.split_numpy(x, ref, width, block, op))


# ---- the plan and the mapping, sanitized ------------------------------------------------------------------------------------------
def test_plan_and_mapping_in_a_sanitized_program(tmp_path, cases):
    """tests/sim/base_items_san.cpp: rcx_base_items_plan and the functions that map a step, a row, a lane and a rest lane to an
    item's bytes and its base's, in a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer.  Over the whole
    case list, split and join, with grids that loop: every byte of every item is read once and written once, nothing else is
    touched, the base is read inside the items' spans only, and without base items the typed tables are rcx_typed_plan's."""
    exe, text = str(tmp_path / "base_items_san"), str(tmp_path / "cases.txt")
    bc.write_cases(text, cases + typed_only())
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "base_items_san.cpp")], check=True)
    r = subprocess.run([exe, text], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "base_items_san ok: 55 batches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def typed_only():
    """The 25 batches of the typed item tests as batches without an op: there the typed tables must be rcx_typed_plan's."""
    out = []
    for k, c in enumerate(tc.kernel_cases()):
        out.append(dict(c, ops=np.full(len(c["widths"]), bc.NO_BASE, np.uint8), layout="packed", base_offset=0))
    return out


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_base_items.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, rcx, stats, stored, stored_items
    build.build()
    names = declared_symbols()
    assert len(names) == 6 and set(names) == set(bi.EXPORTS), (names, bi.EXPORTS)
    for name in names:
        assert getattr(bi.lib(), name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "rcx_base_items.h")).read()
    assert '#include "rcx_base.h"' in text and '#include "rcx_typed_items.h"' in text
    # rcx.h and the other headers are what they were, and no name is shared
    assert len(rcx.EXPORTS) == 57 and len(base.EXPORTS) == 4 and len(typed_items.EXPORTS) == 6 and rcx.lib().rcx_version() == 300
    others = set(rcx.EXPORTS)
    for module in (planes, predict, stats, stored, stored_items, typed_items, base):
        others |= set(module.EXPORTS)
    assert not set(bi.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_base_items.hpp", "rcx_base_items_api.hpp")) and any(h.endswith("rcx_base_items.h") for h in build.HEADERS)
    api = open(os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_api.hip")).read()
    assert '#include "rcx_base_items_api.hpp"' in api
    # the sub-items are rcx_typed_items.h's: the stage declares no table of its own
    assert not any("sub" in name for name in names)
    # the two pure functions, which need no GPU
    assert bi.check(*EXAMPLE, [2, 0xFF]) == rcx.OK and bi.hull(*EXAMPLE, [2, 0xFF]) == (2, 9)
    assert bi.check(*EXAMPLE, [2, 1]) == rcx.E_ARG and bi.check(*EXAMPLE, [4, 0xFF]) == rcx.E_ARG and bi.check(EXAMPLE[0], None, *EXAMPLE[2:], [2, 0xFF]) == rcx.E_ARG
    assert bi.check(EXAMPLE[0], None, *EXAMPLE[2:], None) == rcx.OK and bi.hull(EXAMPLE[0], None, *EXAMPLE[2:], None) == (0, 0)


# ---- RCXK --------------------------------------------------------------------------------------------------------------------
LENGTHS, WIDTHS, PREDS, OPS = [9, 0, 16, 5], [2, 4, 8, 1], [0, 0, 1, 0], [2, 0, 0xFF, 0xFF]
SUB_OFFS = np.concatenate([[0], np.cumsum([3, 4] + [0] * 4 + [1] * 8 + [2])]).astype(np.uint64)
BASE_CRCS = np.array([0xCBF43926, 0, 0, 0], np.uint32)


def inner_blob(preds=PREDS, crcs=None, lengths=LENGTHS, directory=b"dir"):
    return container.typed_items_header_bytes(2, lengths, WIDTHS, preds, SUB_OFFS, crcs, directory) + bytes(int(SUB_OFFS[-1]))


def delta_items_blob(ops=OPS, base_crcs=None, inner=None):
    return container.delta_items_header_bytes(ops, base_crcs) + (inner_blob() if inner is None else inner)


def test_every_layout_name_is_a_name_of_the_container():
    for name in ("DELTA_ITEMS_MAGIC", "DELTA_ITEMS_VERSION", "DELTA_ITEMS_FLAG_BASE_CRC", "BASE_OP_NONE", "delta_items_header_bytes", "parse_delta_items",
                 "BaseItemMismatchError"):
        assert getattr(container, name) is getattr(layout, name)
    assert container.DELTA_ITEMS_MAGIC == b"RCXK" and container.DELTA_ITEMS_VERSION == 1 and container.BASE_OP_NONE == 0xFF
    e = container.BaseItemMismatchError(7, "w")
    assert isinstance(e, container.BaseMismatchError) and isinstance(e, container.ContainerError) and (e.index, e.name) == (7, "w")
    assert "item 7" in str(e) and "'w'" in str(e) and "tensor" not in str(container.BaseItemMismatchError(3))
    assert "RCXK" in layout.__doc__ and "RCXK" in container.__doc__


def test_layout_byte_for_byte():
    blob = delta_items_blob(base_crcs=BASE_CRCS)
    assert blob[:16] == b"RCXK" + bytes([1, 1, 0, 0]) + struct.pack("<Q", 4)
    assert blob[16:20] == bytes([2, 0, 0xFF, 0xFF]) and blob[20:36] == struct.pack("<4I", 0xCBF43926, 0, 0, 0)
    assert blob[36:] == inner_blob() and blob[36:40] == b"RCXJ"
    plain = delta_items_blob()
    assert plain[:16] == b"RCXK" + bytes([1, 0, 0, 0]) + struct.pack("<Q", 4) and plain[20:] == inner_blob()
    for b, crcs, at in ((blob, BASE_CRCS, 36), (plain, None, 20)):
        c = container.parse_delta_items(b)
        assert c["nitems"] == 4 and c["ops"].tolist() == OPS and c["inner_at"] == at and c["flags"] == (crcs is not None)
        assert (c["base_crcs"] is None) if crcs is None else np.array_equal(c["base_crcs"], crcs)
        assert c["inner"]["directory"] == b"dir" and c["inner"]["preds"].tolist() == PREDS and c["inner"]["coder"] == 2
        assert c["inner"]["payload"].tobytes() == bytes(int(SUB_OFFS[-1]))
    # whatever the inner container carries, it carries here
    checked = delta_items_blob(inner=inner_blob(crcs=np.arange(15, dtype=np.uint32)))
    assert container.parse_delta_items(checked)["inner"]["crcs"].tolist() == list(range(15))
    empty = container.delta_items_header_bytes([], np.zeros(0, np.uint32)) + container.typed_items_header_bytes(0, [], [], [], [0])
    assert container.parse_delta_items(empty)["nitems"] == 0


def test_refusals():
    good = delta_items_blob(base_crcs=BASE_CRCS)

    def patched(at, value):
        return good[:at] + bytes(value) + good[at + len(value):]

    for bad, why in ((patched(4, [2]), "version"), (patched(4, [0]), "version"), (patched(5, [2]), "flag"), (patched(5, [3]), "flag"), (patched(5, [0x81]), "flag"),
                     (patched(6, [1]), "reserved"), (patched(7, [1]), "reserved"), (patched(16, [3]), "op"), (patched(17, [0xFE]), "op"),
                     (patched(36, b"RCXI"), "inner magic"), (patched(36, b"RCXT"), "inner magic"), (patched(36, b"RCXK"), "inner magic"),
                     (patched(8, struct.pack("<Q", 3)), "nitems"), (patched(8, struct.pack("<Q", 1 << 63)), "nitems"), (good[:30], "truncated"),
                     (good[:12], "truncated"), (good[:36], "no inner container"), (good + b"x", "payload"),
                     (delta_items_blob([2, 0, 0, 0xFF], None), "a predictor on an item with an op"),
                     (delta_items_blob(inner=inner_blob([2, 0, 1, 0])), "a predictor on an item with an op"),
                     (container.delta_items_header_bytes(OPS[:3]) + inner_blob(), "nitems")):
        with pytest.raises(container.ContainerError):
            container.parse_delta_items(bad)
            pytest.fail(why)
    for bad in (lambda: container.delta_items_header_bytes([0, 3]), lambda: container.delta_items_header_bytes(OPS, BASE_CRCS[:3]),
                lambda: container.delta_items_header_bytes(OPS, [1, 0, 5, 0])):  # a checksum for an item without a base
        with pytest.raises(container.ContainerError):
            bad()
    # the five other parsers refuse it by its magic, and it refuses theirs
    for parse in (container.parse, container.parse_items, container.parse_typed, container.parse_typed_items, container.parse_delta):
        with pytest.raises(container.ContainerError, match="not an RCX"):
            parse(good)
    with pytest.raises(container.ContainerError, match="not an RCXK"):
        container.parse_delta_items(inner_blob())


def test_what_the_calls_refuse_before_they_need_a_gpu():
    x, b = np.arange(8, dtype=np.uint16), np.arange(8, dtype=np.uint16)
    E = container.ContainerError
    for bad in (lambda: container.pack_delta_items([x], [b[:7]]), lambda: container.pack_delta_items([x], [b.astype(np.uint32)]),      # a base of another length
                lambda: container.pack_delta_items([x], []), lambda: container.pack_delta_items([x, x], [b, None], ops=["sub", "sub"]),  # an op and no base
                lambda: container.pack_delta_items([x], [b], ops="auto"), lambda: container.pack_delta_items([x], [b], ops=[2]),
                lambda: container.pack_delta_items([x, x], [b, None], ops=["sub"]),
                lambda: container.pack_delta_items([x, x], [b, None], predict=["delta", None]),                                    # an explicit predictor AND a base
                lambda: container.pack_delta_items([x.tobytes()], [b]), lambda: container.pack_delta_items([x], [b], widths=3),
                lambda: container.pack_delta_items([x], [b], stored=2.0)):
        with pytest.raises(E):
            bad()
    blob = delta_items_blob(base_crcs=BASE_CRCS)
    for bad in (lambda: container.unpack_delta_items(blob, [None] * 3), lambda: container.unpack_delta_items(blob, [None] * 4, pick=[4]),
                lambda: container.unpack_delta_items(blob, [None] * 4),                       # item 0 was packed against a base
                lambda: container.unpack_delta_items(blob, [bytes(8), None, None, None])):    # ... of 9 bytes
        with pytest.raises(E):
            bad()
    assert container.unpack_delta_items(blob, [None] * 4, pick=[]) == [] and container.unpack_delta_items(blob, [None] * 4, pick=[1, 1]) == [b"", b""]
    named = {"a": np.arange(8, dtype=np.float32)}
    for bad in (lambda: container.pack_tensors_delta(named, {}, op={"a": "sub"}), lambda: container.pack_tensors_delta(named, {"a": named["a"][:7]}, op={"a": "sub"}),
                lambda: container.pack_tensors_delta(named, {"a": named["a"].astype(np.int32)}, op={"a": "sub"}),
                lambda: container.pack_tensors_delta(named, named, block=8), lambda: container.pack_tensors_delta(named, named, op="minus"),
                lambda: container.pack_tensors_delta({"a": np.zeros(3, np.complex128)}, {})):
        with pytest.raises(E):
            bad()
    # nothing to code: no GPU, and the container round-trips through the parser
    blob = container.pack_tensors_delta({"e": np.zeros((0, 3), np.float32)}, {"e": np.zeros((0, 3), np.float32)})
    c = container.parse_delta_items(blob)
    assert c["nitems"] == 0 and container.parse_tensor_directory(c["inner"]["directory"], 0)[0]["shape"] == (0, 3)
    assert container.pack_delta_items([b"", x[:0]], [None, b[:0]], widths=[1, 2])[:24] == b"RCXK" + bytes([1, 1, 0, 0]) + struct.pack("<Q", 2) + bytes([0xFF, 2]) + bytes(6)


# ---- why it exists, with the CPU oracle ------------------------------------------------------------------------------------------
BLOCK = 65536


def oracle_container(oracle, t, delta: bool):
    """The RCXK (delta) or the RCXJ of the same items (ops dropped) that the device path writes, made with the twin and the CPU
    oracle -> (blob, payload bytes per item)"""
    offs = np.concatenate([[0], np.cumsum(t["lengths"])]).astype(np.uint64)
    ops = t["ops"] if delta else None
    y = bi.split_numpy(t["x"], t["ref"], offs, t["base_offsets"], t["widths"], t["preds"], ops)
    soffs = typed_items.sub_offsets_numpy(offs, t["widths"]).astype(np.int64)
    payload, offsets = sic.oracle_item_streams(oracle, [y[soffs[k]: soffs[k + 1]] for k in range(len(soffs) - 1)], 0)
    inner = container.typed_items_header_bytes(0, t["lengths"], t["widths"], t["preds"], offsets, None, b"") + payload.tobytes()
    per_sub = np.diff(offsets.astype(np.int64))
    first = np.concatenate([[0], np.cumsum(t["widths"].astype(np.int64))])
    per_item = np.array([per_sub[first[i]: first[i + 1]].sum() for i in range(len(t["widths"]))])
    if not delta:
        return inner, per_item
    crcs = [zlib.crc32(t["ref"][int(b): int(b) + int(n)].tobytes()) if op != bc.NO_BASE else 0 for b, n, op in zip(t["base_offsets"], t["lengths"], t["ops"])]
    return container.delta_items_header_bytes(t["ops"], crcs) + inner, per_item


# measured with the CPU oracle; README.md and DESIGN.md section 18 quote them.  The dict has 1 572 864 bytes.
PINNED = {"rcxk": 432_890, "rcxj": 1_053_412, "layer0.weight": 120_417, "layer1.weight": 90_099, "embed.frozen": 1_244, "head.new": 110_709,
          "index.sorted": 109_991}


def test_a_state_dict_against_the_one_before_it(oracle):
    """The crafted state dict of the documents (tests/base_items_cases.py: state_dicts), adaptive coder, 64 KiB blocks."""
    named, before, predict = bc.state_dicts()
    t = bc.tensor_items(named, before, BLOCK, bi.SUBZZ, predict)
    assert t["ops"].tolist() == [2] * 4 + [2] * 3 + [2] * 1 + [0xFF] * 2 and t["preds"].tolist() == [0] * 9 + [1]
    rcxk, per_item = oracle_container(oracle, t, True)
    rcxj, plain = oracle_container(oracle, t, False)
    c = container.parse_delta_items(rcxk)
    assert c["ops"].tolist() == t["ops"].tolist() and c["inner"]["nsub"] == 2 * 7 + 4 + 2 + 8
    sizes = {"rcxk": len(rcxk), "rcxj": len(rcxj)}
    for name, first in t["first"].items():
        count = -(-named[name].nbytes // (named[name].dtype.itemsize * BLOCK))
        sizes[name] = int(per_item[first: first + count].sum())
    print(sizes, plain.tolist())
    assert len(rcxk) < len(rcxj)                                          # the whole container, prefix and guard included
    assert sizes["embed.frozen"] * 32 < named["embed.frozen"].nbytes       # all zeros: four blocks of 64 KiB at about 0.5 KiB each
    assert sizes["head.new"] == int(plain[8]) and sizes["index.sorted"] == int(plain[9])  # without a base, what they were
    assert sizes == PINNED


def test_one_tensor_carries_the_payload_of_the_delta_container(oracle):
    """The 1 Mi bf16 checkpoint pair of the RCXD documents as ONE tensor against its base: the sub-items are RCXD's blocks and
    the streams are the same streams, 481 700 bytes of them."""
    w2, w, _ = base_cases.checkpoint_pair()
    t = bc.tensor_items({"w": w2.view(np.uint16)}, {"w": w.view(np.uint16)}, BLOCK, bi.SUBZZ)
    assert len(t["lengths"]) == 16 and t["ops"].tolist() == [2] * 16
    blob, per_item = oracle_container(oracle, t, True)
    assert int(per_item.sum()) == 481_700 == len(container.parse_delta_items(blob)["inner"]["payload"])
