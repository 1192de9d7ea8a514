"""The byte-plane filter as far as it goes without a GPU: the numpy restatement pinned by the worked vectors of
include/rcx_planes.h, the header against planes.EXPORTS and the built library, the RCXT header, the command line, and with the
CPU oracle the reason the filter exists -- typed data codes smaller by planes."""
import os
import re
import struct

import numpy as np
import pytest

import planes_cases as pc
from cpprcoder_amd import container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_worked_vectors_pin_the_restatement():
    assert list(pc.split_numpy(np.arange(10, dtype=np.uint8), 4, 16)) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 9]
    want = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 32, 34, 33, 35, 36]
    assert list(pc.split_numpy(np.arange(37, dtype=np.uint8), 2, 16)) == want
    assert list(pc.join_numpy(np.array(want, np.uint8), 2, 16)) == list(range(37))
    assert list(pc.join_numpy(np.array([0, 4, 1, 5, 2, 6, 3, 7, 8, 9], np.uint8), 4, 16)) == list(range(10))
    # a whole superblock: coder block s * w + p is plane p
    x = np.random.RandomState(1).randint(0, 256, 2 * 4 * 48 + 7, dtype=np.uint8)
    y = pc.split_numpy(x, 4, 48)
    for s in range(2):
        for p in range(4):
            assert np.array_equal(y[(4 * s + p) * 48: (4 * s + p + 1) * 48], x[s * 192 + p: (s + 1) * 192: 4])
    assert np.array_equal(y[384:], x[384:])  # one whole element (four planes of one byte) and three tail bytes: as they were


def test_join_inverts_split_over_the_shape_list():
    rs = np.random.RandomState(2)
    cases = pc.kernel_cases()
    assert {c[0] for c in cases} == set(pc.WIDTHS) and {c[1] for c in cases} == set(pc.BLOCKS)
    for side in (3, 4):  # every offset on both sides, at B = 100 too
        assert {c[side] for c in cases} == set(pc.OFFSETS) and {c[side] for c in cases if c[1] == 100} == set(pc.OFFSETS)
    for width, block, n, _, _ in cases:
        x = rs.randint(0, 256, n, dtype=np.uint8)
        y = pc.split_numpy(x, width, block)
        assert np.array_equal(pc.join_numpy(y, width, block), x), (width, block, n)
        assert np.array_equal(np.sort(y), np.sort(x))


def test_a_span_between_superblock_borders_transforms_alone():
    x = np.random.RandomState(3).randint(0, 256, 5 * 8 * 100 + 61, dtype=np.uint8)
    y = pc.split_numpy(x, 8, 100)
    for lo, hi in ((0, 800), (800, 2400), (1600, len(x)), (4000, len(x))):
        assert np.array_equal(pc.split_numpy(x[lo:hi], 8, 100), y[lo:hi])
        assert np.array_equal(pc.join_numpy(y[lo:hi], 8, 100), x[lo:hi])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_planes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, rcx
    build.build()
    names = declared_symbols()
    assert len(names) == 4 and set(names) == set(planes.EXPORTS), (names, planes.EXPORTS)
    for name in names:
        assert getattr(planes.lib(), name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "rcx_planes.h")).read()
    assert '#include "rcx.h"' in text
    # rcx.h itself is what it was: no new function, the same version
    assert len(rcx.EXPORTS) == 57 and not set(planes.EXPORTS) & set(rcx.EXPORTS) and rcx.lib().rcx_version() == 300
    assert all(h in build.HEADERS for h in ("rcx_planes.hpp", "rcx_predict.hpp", "rcx_typed_api.hpp"))  # (one kernel template, one API file)


# ---- the RCXT header -----------------------------------------------------------------------------------------------------------
OFFS = np.array([0, 100, 250, 251], np.uint64)
N3 = 3 * 4096 - 7


def typed_blob(crcs=None, width=4):
    return container.typed_header_bytes(2, 4096, N3, width, OFFS, crcs) + bytes(251)


def test_typed_header_round_trips():
    c = container.parse_typed(typed_blob())
    assert (c["coder"], c["flags"], c["block"], c["n"], c["nblocks"], c["width"]) == (2, 0, 4096, N3, 3, 4)
    assert c["crcs"] is None and np.array_equal(c["offsets"], OFFS) and len(c["payload"]) == 251
    crcs = np.array([0xCBF43926, 0, 0xFFFFFFFF], np.uint32)
    c = container.parse_typed(typed_blob(crcs, width=8))
    assert c["flags"] == container.FLAG_CRC32 and c["width"] == 8 and c["crcs"].dtype == np.uint32 and np.array_equal(c["crcs"], crcs)
    c = container.parse_typed(container.typed_header_bytes(0, 65536, 0, 2, np.zeros(1, np.uint64), np.zeros(0, np.uint32)))
    assert c["n"] == 0 and c["nblocks"] == 0 and len(c["crcs"]) == 0 and len(c["payload"]) == 0


def test_typed_header_layout_byte_for_byte():
    fixed = struct.pack("<4sBBHIQQB7s", b"RCXT", 1, 2, 0, 4096, N3, 3, 4, bytes(7))
    assert len(fixed) == 36 and typed_blob() == fixed + OFFS.astype("<u8").tobytes() + bytes(251)
    crcs = np.array([1, 2, 3], np.uint32)
    fixed = struct.pack("<4sBBHIQQB7s", b"RCXT", 1, 2, 2, 4096, N3, 3, 4, bytes(7))
    assert typed_blob(crcs) == fixed + OFFS.astype("<u8").tobytes() + crcs.astype("<u4").tobytes() + bytes(251)
    assert typed_blob(crcs)[28] == 4 and typed_blob(crcs)[4] == 1  # the width's place; version 1 with or without checksums


def test_typed_header_refusals():
    blob, checked = typed_blob(), typed_blob(np.array([1, 2, 3], np.uint32))
    table_end = 36 + 8 * 4

    def with_byte(b, at, value):
        out = bytearray(b)
        out[at] = value
        return bytes(out)

    bad = [with_byte(blob, 28, w) for w in (1, 3, 16, 0)]                                  # the width
    bad += [with_byte(blob, at, 1) for at in range(29, 36)]                                # each reserved byte
    bad += [with_byte(blob, 6, 4), with_byte(checked, 6, 6), with_byte(blob, 6, 1), with_byte(blob, 7, 1)]  # unknown flags (the block sort's too)
    bad += [with_byte(blob, 4, 2), with_byte(checked, 4, 2), with_byte(blob, 4, 0)]         # versions
    bad += [with_byte(blob, 5, 4), with_byte(blob, 6, 2)]                                  # coder; the CRC flag without its table
    bad += [blob + b"x", blob[:-1], checked + b"x", blob[: table_end - 1], blob[:36], blob[:35], checked[: table_end + 11], checked[: table_end]]
    for damaged in bad:
        with pytest.raises(container.ContainerError):
            container.parse_typed(damaged)
    for width in (1, 3, 16):
        with pytest.raises(container.ContainerError):
            typed_blob(width=width)
    with pytest.raises(container.ContainerError):
        typed_blob(np.array([1, 2], np.uint32))  # one checksum per block
    # the three containers do not read each other's files
    rcxb = container.header_bytes(2, 4096, N3, OFFS) + bytes(251)
    rcxi = container.item_header_bytes(0, [100, 0, 7], [0, 60, 60, 75]) + bytes(75)
    for other in (rcxb, rcxi):
        with pytest.raises(container.ContainerError):
            container.parse_typed(other)
    for b in (blob, checked):
        with pytest.raises(container.ContainerError):
            container.parse(b)
        with pytest.raises(container.ContainerError):
            container.parse_items(b)


def test_what_pack_typed_refuses_before_it_needs_a_gpu():
    for data, width in ((b"abcdefgh", None), (b"abcdefgh", 1), (b"abcdefgh", 3), (np.zeros(8, np.uint8), None), (np.zeros(4, np.complex128), None)):
        with pytest.raises(container.ContainerError):
            container.pack_typed(data, width)
    torch = pytest.importorskip("torch")
    with pytest.raises(container.ContainerError):
        container.pack_typed(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(container.ContainerError):
        container.pack_typed(torch.zeros(4, 4)[:, 1])  # not contiguous
    # nothing to code: a header and no GPU
    for data in (b"", np.zeros(0, np.float32), torch.zeros(0, dtype=torch.bfloat16)):
        blob = container.pack_typed(data, 4 if isinstance(data, bytes) else None, checksum=True)
        assert container.parse_typed(blob)["n"] == 0 and container.unpack_typed(blob) == b""
    assert container.parse_typed(container.pack_typed(torch.zeros(0, dtype=torch.bfloat16)))["width"] == 2


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_command_line_takes_planes():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    a = ap.parse_args(["c", "--planes", "4", "--crc", "in", "out"])
    assert a.planes == 4 and a.crc and not a.blksort and ap.parse_args(["c", "in", "out"]).planes is None
    assert ap.parse_args(["t", "--planes", "2", "f"]).planes == 2 and ap.parse_args(["t", "--blksort", "f"]).planes is None
    for argv in (["c", "--planes", "3", "in", "out"], ["c", "--planes", "2", "--blksort", "in", "out"], ["t", "--blksort", "--planes", "8", "f"],
                 ["d", "--planes", "2", "in", "out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)


# ---- the benefit, with the CPU oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_float_tensors_code_smaller_by_planes(oracle, name):
    """1 MiB of randn(12345) * 0.02: at both block sizes, every coder's total is strictly smaller behind the filter
    (the ratios are 0.86 .. 0.94)."""
    x, width = pc.randn_bytes(name)
    assert len(x) == 1 << 20
    for block in (65536, 4096):
        y = pc.split_numpy(x, width, block)
        for coder in (0, 1, 2, 3):
            plain, planar = pc.total_size(oracle, x, block, coder), pc.total_size(oracle, y, block, coder)
            print(name, block, coder, plain, planar, round(planar / plain, 4))
            assert planar < plain, (name, block, coder, plain, planar)


def test_indices_code_smaller_by_planes_except_with_rans8(oracle):
    """int64 indices below 50 000: five constant planes of eight.  The adaptive, static and one-state rANS coders gain;
    the eight-state rANS coder pays 2 bytes a symbol for a plane of one repeated byte (the reference's behaviour for a
    frequency of 4096, include/rcx.h at rcx_block_bound_for), so all that is asserted of it is that it fits its bound."""
    x, width = pc.index_bytes()
    for block in (65536, 4096):
        y = pc.split_numpy(x, width, block)
        for coder in (0, 1, 2):
            plain, planar = pc.total_size(oracle, x, block, coder), pc.total_size(oracle, y, block, coder)
            print("int64", block, coder, plain, planar, round(planar / plain, 4))
            assert planar < plain, (block, coder, plain, planar)
        planar = pc.total_size(oracle, y, block, 3)
        nblocks = -(-len(y) // block)
        print("int64", block, 3, pc.total_size(oracle, x, block, 3), planar)
        assert planar <= nblocks * oracle.block_bound(block, 3) + 16  # rcx_encode_bound_for
