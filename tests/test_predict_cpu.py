"""The delta predictor as far as it goes without a GPU: the numpy restatement pinned by the worked vectors of
include/rcx_predict.h, the kernels' per-unit arithmetic compiled for the host against a scalar loop, the header against
predict.EXPORTS and the built library, RCXT version 2, the command line, and with the CPU oracle the reason the predictor
exists -- integers with small differences code smaller by it."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import planes_cases as pc
import predict_cases as pr
from cpprcoder_amd import container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_SRC = os.path.join(ROOT, "tests", "sim", "predict_sim.cpp")
SIM_SO = os.path.join(ROOT, "tests", "sim", "libpredictsim.so")

VECTOR = bytes.fromhex("0100030006 00FFFF0200AA".replace(" ", ""))  # the elements 1, 3, 6, 65535, 2 and one tail byte


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_worked_vectors_pin_the_restatement():
    x = np.frombuffer(VECTOR, np.uint8)
    assert list(x[:10].view("<u2")) == [1, 3, 6, 65535, 2]
    assert list(pr.predict_numpy(x, 2, 16, pr.DELTA)[:10].view("<u2")) == [1, 2, 3, 0xFFF9, 3]
    assert list(pr.predict_numpy(x, 2, 16, pr.ZIGZAG)[:10].view("<u2")) == [2, 4, 6, 13, 6]
    assert pr.split_numpy(x, 2, 16, pr.DELTA).tobytes() == bytes.fromhex("0102 03F9 0300 0000 FF00 AA".replace(" ", ""))
    assert pr.split_numpy(x, 2, 16, pr.ZIGZAG).tobytes() == bytes.fromhex("0204 060D 0600 0000 0000 AA".replace(" ", ""))
    assert pr.split_numpy(x, 2, 16, pr.NONE).tobytes() == pc.split_numpy(x, 2, 16).tobytes()
    for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG):
        assert pr.join_numpy(pr.split_numpy(x, 2, 16, pred), 2, 16, pred).tobytes() == VECTOR
    # the predictor restarts in every superblock: the first element of the second one stays what it is
    e = np.array([10, 11, 13, 16] * 8 + [1000, 1001, 999], "<u4")
    d = pr.predict_numpy(e.view(np.uint8), 4, 16, pr.DELTA).view("<u4")
    assert list(d[:4]) == [10, 1, 2, 3] and list(d[16:20]) == [10, 1, 2, 3] and list(d[32:]) == [1000, 1, 0xFFFFFFFE]
    z = pr.predict_numpy(e.view(np.uint8), 4, 16, pr.ZIGZAG).view("<u4")
    assert list(z[:4]) == [20, 2, 4, 6] and list(z[32:]) == [2000, 2, 3]
    # zigzag on the edges of each width
    for dtype, bits in (("<u2", 16), ("<u4", 32), ("<u8", 64)):
        top = (1 << bits) - 1
        d = np.array([0, 1, top, 2, top - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1], dtype)
        assert [int(v) for v in pr.zigzag(d)] == [0, 2, 1, 4, 3, top, top - 1]
        assert np.array_equal(pr.unzigzag(pr.zigzag(d)), d)


def test_the_inverse_inverts_over_the_shape_list():
    rs = np.random.RandomState(2)
    cases = pr.kernel_cases()
    assert {c[0] for c in cases} == set(pr.WIDTHS) and {c[1] for c in cases} == set(pr.BLOCKS)
    for side in (3, 4):
        assert {c[side] for c in cases} == set(pr.OFFSETS)
    for width, block, n, _, _ in cases:
        x = rs.randint(0, 256, n, dtype=np.uint8)
        for pred in pr.PREDS:
            y = pr.split_numpy(x, width, block, pred)
            assert len(y) == n and np.array_equal(pr.join_numpy(y, width, block, pred), x), (width, block, n, pred)
    for kind, width in (("minus_k", 2), ("minus_k", 4), ("minus_k", 8), ("ramp", 8)):
        x = pr.kernel_data(kind, width, 3 * width * 100 + 5, None)
        d = pr.predict_numpy(x, width, 100, pr.DELTA)
        if kind == "minus_k":  # every byte of every difference but a superblock's first is 0xFF
            assert bool((d[width: width * 100] == 0xFF).all()) and bool((d[width * 101: width * 200] == 0xFF).all())
        else:
            assert list(x[:80].view("<u8")) == [(1 << 32) - 8 + k for k in range(10)] and bool((d[8:800].view("<u8") == 1).all())
        for pred in pr.PREDS:
            assert np.array_equal(pr.join_numpy(pr.split_numpy(x, width, 100, pred), width, 100, pred), x)


def test_a_span_between_superblock_borders_transforms_alone():
    x = np.random.RandomState(3).randint(0, 256, 5 * 8 * 100 + 61, dtype=np.uint8)
    for pred in pr.PREDS:
        y = pr.split_numpy(x, 8, 100, pred)
        for lo, hi in ((0, 800), (800, 2400), (1600, len(x)), (4000, len(x))):
            assert np.array_equal(pr.split_numpy(x[lo:hi], 8, 100, pred), y[lo:hi])
            assert np.array_equal(pr.join_numpy(y[lo:hi], 8, 100, pred), x[lo:hi])


# ---- the kernels' unit arithmetic on the host ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    csrc = os.path.join(ROOT, "cpprcoder_amd", "csrc")
    deps = [SIM_SRC] + [os.path.join(csrc, f) for f in ("rcx_predict.hpp", "rcx_planes.hpp", "rcx_lane.hpp")]
    if not os.path.exists(SIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SIM_SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SIM_SO, SIM_SRC], check=True)
    L = C.CDLL(SIM_SO)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.sim_predict_units.restype, L.sim_predict_units.argtypes = C.c_int, [vp, vp, u32, u32, u32, vp]
    L.sim_unpredict_units.restype, L.sim_unpredict_units.argtypes = C.c_int, [vp, vp, u32, u32, u32, vp, vp]
    L.sim_zigzag.restype, L.sim_zigzag.argtypes = u64, [u64, u32]
    L.sim_unzigzag.restype, L.sim_unzigzag.argtypes = u64, [u64, u32]
    L.sim_planes_units.restype, L.sim_planes_units.argtypes = C.c_int, [vp, u32, u32, vp]
    return L


def edge_values(width):
    bits = 8 * width
    return [0, (1 << bits) - 1, 1 << (bits - 1), 1, (1 << (bits - 1)) - 1, (1 << bits) - 2, 0x0100 % (1 << bits), (1 << (bits // 2)) - 1, 1 << (bits // 2)]


def sim_units(width):
    """Units of 16 elements: each edge value repeated, the edge values in turn, two rotations of them, and random ones;
    with them an element in front of each unit that runs through the edge values as well."""
    dtype, edges = f"<u{width}", edge_values(width)
    units = [np.full(16, v, np.uint64) for v in edges]
    units += [np.array([edges[(k + r) % len(edges)] for k in range(16)], np.uint64) for r in range(3)]
    rs = np.random.RandomState(40 + width)
    units += [np.frombuffer(rs.bytes(16 * 8), np.uint64) & np.uint64((1 << (8 * width)) - 1) for _ in range(40)]
    e = np.stack(units).astype(dtype)
    fronts = np.array([edges[k % len(edges)] for k in range(len(units))], np.uint64)
    return e, fronts


@pytest.mark.parametrize("width", pr.WIDTHS)
@pytest.mark.parametrize("pred", pr.PREDS)
def test_unit_arithmetic_on_the_host_is_the_scalar_loop(sim, width, pred):
    e, fronts = sim_units(width)
    count, mask = len(e), (1 << (8 * width)) - 1
    want = np.zeros_like(e)
    for u in range(count):  # the scalar loop, in Python integers
        front = int(fronts[u])
        for k in range(16):
            d = (int(e[u, k]) - front) & mask
            want[u, k] = ((d << 1) ^ (0 - (d >> (8 * width - 1)))) & mask if pred == pr.ZIGZAG else d
            front = int(e[u, k])
    got = np.zeros_like(e)
    assert sim.sim_predict_units(e.ctypes.data, fronts.ctypes.data, count, width, int(pred == pr.ZIGZAG), got.ctypes.data) == 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # the inverse: the scan of a unit plus what lies in front of it gives the elements back, and the unit's total
    back, totals = np.zeros_like(e), np.zeros(count, np.uint64)
    assert sim.sim_unpredict_units(want.ctypes.data, fronts.ctypes.data, count, width, int(pred == pr.ZIGZAG), back.ctypes.data, totals.ctypes.data) == 0
    assert np.array_equal(back, e), np.argwhere(back != e)[:4]
    assert [int(t) for t in totals] == [(int(e[u, 15]) - int(fronts[u])) & mask for u in range(count)]
    for v in edge_values(width) + [int(x) for x in e[-1]]:
        z = sim.sim_zigzag(v, width)
        assert z == ((v << 1) ^ (0 - (v >> (8 * width - 1)))) & mask and sim.sim_unzigzag(z, width) == v
    # and the transpose both kernels reuse, on the same units
    planes = np.zeros((count, 16 * width), np.uint8)
    assert sim.sim_planes_units(e.ctypes.data, count, width, planes.ctypes.data) == 1
    assert np.array_equal(planes.reshape(-1), pc.split_numpy(e.view(np.uint8).reshape(-1), width, 16))


def test_unit_arithmetic_in_a_sanitized_program(tmp_path):
    """tests/sim/predict_san.cpp: the same functions in a program of its own under AddressSanitizer and
    UndefinedBehaviorSanitizer (shifts by the width, the sign fold, the packing of 16-bit elements)."""
    exe = str(tmp_path / "predict_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "predict_san.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "predict_san ok" in r.stdout, r.stdout + r.stderr


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_predict.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, rcx
    build.build()
    names = declared_symbols()
    assert len(names) == 4 and set(names) == set(predict.EXPORTS), (names, predict.EXPORTS)
    for name in names:
        assert getattr(predict.lib(), name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "rcx_predict.h")).read()
    assert '#include "rcx_planes.h"' in text
    for name, value in (("NONE", 0), ("DELTA", 1), ("ZIGZAG", 2)):
        assert getattr(predict, name) == value and re.search(rf"#define RCX_PRED_{name} {value}u\b", text)
    # rcx.h and rcx_planes.h are what they were
    assert len(rcx.EXPORTS) == 57 and len(planes.EXPORTS) == 4 and rcx.lib().rcx_version() == 300
    assert not set(predict.EXPORTS) & (set(rcx.EXPORTS) | set(planes.EXPORTS))
    assert all(h in build.HEADERS for h in ("rcx_planes.hpp", "rcx_predict.hpp", "rcx_typed_api.hpp"))
    assert any(h.endswith("rcx_predict.h") for h in build.HEADERS)


# ---- RCXT version 2 ------------------------------------------------------------------------------------------------------------
OFFS = np.array([0, 100, 250, 251], np.uint64)
N3 = 3 * 4096 - 7


def typed_blob(crcs=None, width=4, pred=0):
    return container.typed_header_bytes(2, 4096, N3, width, OFFS, crcs, pred=pred) + bytes(251)


def test_version_two_round_trips_and_version_one_stays():
    for pred in (1, 2):
        c = container.parse_typed(typed_blob(pred=pred))
        assert (c["coder"], c["flags"], c["block"], c["n"], c["nblocks"], c["width"], c["pred"]) == (2, 0, 4096, N3, 3, 4, pred)
        assert c["crcs"] is None and np.array_equal(c["offsets"], OFFS) and len(c["payload"]) == 251
    crcs = np.array([0xCBF43926, 0, 0xFFFFFFFF], np.uint32)
    c = container.parse_typed(typed_blob(crcs, width=8, pred=2))
    assert c["flags"] == container.FLAG_CRC32 and c["width"] == 8 and c["pred"] == 2 and np.array_equal(c["crcs"], crcs)
    # without a predictor: version 1, byte for byte what it was, and parse_typed says 0
    assert typed_blob() == container.typed_header_bytes(2, 4096, N3, 4, OFFS) + bytes(251) and typed_blob()[4] == 1
    assert container.parse_typed(typed_blob())["pred"] == 0 and container.parse_typed(typed_blob(crcs))["pred"] == 0


def test_version_two_layout_byte_for_byte():
    fixed = struct.pack("<4sBBHIQQBB6s", b"RCXT", 2, 2, 0, 4096, N3, 3, 4, 1, bytes(6))
    assert len(fixed) == 36 and typed_blob(pred=1) == fixed + OFFS.astype("<u8").tobytes() + bytes(251)
    crcs = np.array([1, 2, 3], np.uint32)
    fixed = struct.pack("<4sBBHIQQBB6s", b"RCXT", 2, 2, 2, 4096, N3, 3, 8, 2, bytes(6))
    blob = typed_blob(crcs, width=8, pred=2)
    assert blob == fixed + OFFS.astype("<u8").tobytes() + crcs.astype("<u4").tobytes() + bytes(251)
    assert (blob[4], blob[28], blob[29], blob[30:36]) == (2, 8, 2, bytes(6))
    fixed = struct.pack("<4sBBHIQQB7s", b"RCXT", 1, 2, 0, 4096, N3, 3, 4, bytes(7))
    assert typed_blob(pred=0) == fixed + OFFS.astype("<u8").tobytes() + bytes(251)


def test_version_two_refusals():
    def with_byte(b, at, value):
        out = bytearray(b)
        out[at] = value
        return bytes(out)

    v1, v2 = typed_blob(), typed_blob(pred=1)
    bad = [with_byte(v2, 29, 0), with_byte(v2, 29, 3), with_byte(v2, 29, 255)]       # version 2 names a predictor it knows
    bad += [with_byte(v2, at, 1) for at in range(30, 36)]                           # each reserved byte
    bad += [with_byte(v1, 29, 1), with_byte(v1, 29, 2), with_byte(v1, 4, 2)]         # version 1 has none; version 2 without one
    bad += [with_byte(v2, 4, 3), with_byte(v2, 4, 0), with_byte(v2, 28, 3), with_byte(v2, 6, 1), with_byte(v2, 6, 2), v2 + b"x", v2[:-1], v2[:35]]
    for damaged in bad:
        with pytest.raises(container.ContainerError):
            container.parse_typed(damaged)
    assert container.parse_typed(with_byte(v2, 29, 2))["pred"] == 2  # (and the other one it knows)
    for pred in (3, -1, 256, True, "1", 1.0):
        with pytest.raises(container.ContainerError):
            typed_blob(pred=pred)
    for parse in (container.parse, container.parse_items):  # the other containers do not read it
        with pytest.raises(container.ContainerError):
            parse(v2)


def test_what_pack_typed_refuses_before_it_needs_a_gpu():
    ints = np.arange(64, dtype=np.int64)
    for predict in ("xor", "none", 1, 2, True, "DELTA", ["delta"], b"delta"):
        with pytest.raises(container.ContainerError):
            container.pack_typed(ints, predict=predict)
    for data, width in ((b"abcdefgh", None), (b"abcdefgh", 3), (np.zeros(8, np.uint8), None)):
        with pytest.raises(container.ContainerError):
            container.pack_typed(data, width, predict="delta")
    # nothing to code: a version 2 header and no GPU
    for predict, pred in (("delta", 1), ("zigzag", 2)):
        blob = container.pack_typed(np.zeros(0, np.int32), predict=predict, checksum=True)
        c = container.parse_typed(blob)
        assert (c["n"], c["width"], c["pred"], blob[4]) == (0, 4, pred, 2) and container.unpack_typed(blob) == b""
    assert container.pack_typed(np.zeros(0, np.int32), predict=None) == container.pack_typed(np.zeros(0, np.int32))


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_command_line_takes_a_predictor_with_planes():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    a = ap.parse_args(["c", "--planes", "8", "--predict", "delta", "--crc", "in", "out"])
    assert a.planes == 8 and a.predict == "delta" and a.crc
    assert ap.parse_args(["t", "--planes", "4", "--predict", "zigzag", "f"]).predict == "zigzag"
    assert ap.parse_args(["c", "--planes", "4", "in", "out"]).predict is None and ap.parse_args(["t", "f"]).predict is None
    for argv in (["c", "--predict", "delta", "in", "out"], ["t", "--predict", "zigzag", "f"], ["c", "--blksort", "--predict", "delta", "in", "out"],
                 ["c", "--planes", "4", "--predict", "xor", "in", "out"], ["c", "--planes", "4", "--predict", "in", "out"],
                 ["d", "--predict", "delta", "in", "out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)


# ---- the benefit, with the CPU oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def totals(oracle):
    """(buffer, block, coder, pred) -> the bytes of the compacted block streams, computed once."""
    out = {}
    for name in pr.INTEGER_BUFFERS:
        x, width = pr.integer_bytes(name)
        assert len(x) == 1 << 20
        for block in (65536, 4096):
            for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG):
                y = pr.split_numpy(x, width, block, pred)
                for coder in (0, 1, 2, 3):
                    out[(name, block, coder, pred)] = pc.total_size(oracle, y, block, coder)
    return out


@pytest.mark.parametrize("name", pr.INTEGER_BUFFERS)
def test_integers_with_small_differences_code_smaller_by_the_predictor(totals, name):
    """1 MiB each of sorted keys, CSR offsets, a random walk and a sampled signal: at both block sizes and with the adaptive,
    static and one-state rANS coders, delta + planes is strictly smaller than planes alone, and for the random walk zigzag
    is strictly smaller than delta."""
    for block in (65536, 4096):
        for coder in (0, 1, 2):
            planes_only, delta, zz = (totals[(name, block, coder, pred)] for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG))
            print(name, block, coder, planes_only, delta, zz, round(delta / planes_only, 4), round(zz / planes_only, 4))
            assert delta < planes_only, (name, block, coder, planes_only, delta)
            if name == "random_walk":
                assert zz < delta, (block, coder, delta, zz)


def test_the_table_of_the_design_document(totals):
    """The adaptive coder at 64 KiB blocks: DESIGN.md section 12 quotes these."""
    got = {name: tuple(totals[(name, 65536, 0, pred)] for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG)) for name in pr.INTEGER_BUFFERS}
    print(got)
    assert got == {"sorted_keys": (477361, 239262, 239371), "csr_offsets": (348207, 103173, 103173), "random_walk": (478932, 353355, 255068),
                   "signal": (908411, 579224, 584026)}


def test_rans8_stays_inside_its_bound(totals, oracle):
    """The eight-state rANS coder pays 2 bytes a symbol for a plane of one repeated byte (include/rcx_planes.h), and the
    predictor makes more such planes: all that is asserted of it is that it fits its bound."""
    for name in pr.INTEGER_BUFFERS:
        for block in (65536, 4096):
            nblocks = -(-(1 << 20) // block)
            for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG):
                size = totals[(name, block, 3, pred)]
                print(name, block, 3, pred, size)
                assert size <= nblocks * oracle.block_bound(block, 3) + 16  # rcx_encode_bound_for
