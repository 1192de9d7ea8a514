"""Residuals against a base as far as they go without a GPU: the numpy twin pinned by the worked example of
include/rcx_base.h, the kernel's per-unit word arithmetic compiled for the host in a sanitized program of its own against the
twin, the header against base.EXPORTS and the built library, the RCXD layout and its refusals, the command line, and with the
CPU oracle the reason the stage exists -- a checkpoint codes to less than half against the one before it, and to more against
an unrelated one."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import base_cases as bc
import planes_cases as pc
from cpprcoder_amd import base, container, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = bytes.fromhex("0501 0001 4200 AA".replace(" ", ""))  # the elements 0x0105, 0x0100, 0x0042 and one tail byte
BASE = bytes.fromhex("0001 0201 4200 55".replace(" ", ""))    # the elements 0x0100 (below), 0x0102 (above), 0x0042 (equal)


# ---- the transform -----------------------------------------------------------------------------------------------------------
def test_worked_example_pins_the_twin():
    text = open(os.path.join(ROOT, "include", "rcx_base.h")).read()
    for op, want in ((base.XOR, "05 02 00 00 00 00 AA"), (base.SUB, "05 FE 00 00 FF 00 AA"), (base.SUBZZ, "0A 03 00 00 00 00 AA")):
        y = base.split_numpy(SOURCE, BASE, 2, 16, op)
        assert y.tobytes() == bytes.fromhex(want.replace(" ", "")), (op, y.tobytes().hex())
        assert base.join_numpy(y, BASE, 2, 16, op).tobytes() == SOURCE
        assert want in text  # the header's own bytes
    assert "05 01 00 01 42 00 AA" in text and "00 01 02 01 42 00 55" in text
    # the tail byte is the source's, whatever the base's is; without whole elements nothing changes
    assert base.split_numpy(b"\x07", b"\x09", 2, 16, base.SUB).tobytes() == b"\x07"
    # width 1 has no planes: the residual alone, block by block the same
    x, b = np.arange(40, dtype=np.uint8), np.arange(40, dtype=np.uint8)[::-1].copy()
    assert np.array_equal(base.split_numpy(x, b, 1, 16, base.SUB), x - b) and np.array_equal(base.split_numpy(x, b, 1, 16, base.XOR), x ^ b)
    d = (x - b).astype(np.uint8)
    assert np.array_equal(base.split_numpy(x, b, 1, 16, base.SUBZZ), ((d << 1) ^ (0 - (d >> 7))).astype(np.uint8))
    # against a base of zeros, sub is the plane filter alone
    noise = np.random.RandomState(5).randint(0, 256, 3 * 400 + 7, dtype=np.uint8)
    for width in pc.WIDTHS:
        assert np.array_equal(base.split_numpy(noise, np.zeros_like(noise), width, 100, base.SUB), pc.split_numpy(noise, width, 100))
    for bad in (lambda: base.split_numpy(b"ab", b"a", 2, 16, 0), lambda: base.split_numpy(b"ab", b"ab", 3, 16, 0), lambda: base.join_numpy(b"ab", b"ab", 2, 16, 3)):
        with pytest.raises(ValueError):
            bad()


def test_the_inverse_inverts_over_the_shape_list():
    rs = np.random.RandomState(2)
    cases = bc.kernel_cases()
    assert {c[0] for c in cases} == set(bc.WIDTHS) and {c[1] for c in cases} == set(bc.BLOCKS)
    for side in (3, 4, 5):
        assert {c[side] for c in cases} == set(bc.OFFSETS)
    assert len({c[3:] for c in cases}) > 25  # the three offsets move independently
    for width, block, n, _, _, _ in cases:
        if n > 3 * width * block + 5 and block != 100:
            continue  # (the step sizes once a width are enough here)
        x, b = rs.randint(0, 256, n, dtype=np.uint8), rs.randint(0, 256, n, dtype=np.uint8)
        for op in bc.OPS:
            y = base.split_numpy(x, b, width, block, op)
            assert len(y) == n and np.array_equal(base.join_numpy(y, b, width, block, op), x), (width, block, n, op)
    noise = rs.randint(0, 256, 1 << 14, dtype=np.uint8)
    for kind in bc.KINDS:
        for width in bc.WIDTHS:
            if kind == "straddle" and width != 8:
                continue
            n = 3 * width * 100 + 5
            x, b = bc.kernel_data(kind, width, n, noise)
            assert len(x) == n and len(b) == n
            whole = (n // width) * width if width > 1 else n
            for op in bc.OPS:
                r = pc.join_numpy(base.split_numpy(x, b, width, 100, op), width, 100) if width > 1 else base.split_numpy(x, b, width, 100, op)
                if kind == "equal":
                    assert not r[: 3 * width * 100].any()
                if kind == "minus_one" and op != base.XOR:  # -1: all ones; its zigzag is 1
                    e = r[: 3 * width * 100].view(f"<u{width}")
                    assert bool((e == (1 if op == base.SUBZZ else (1 << (8 * width)) - 1)).all())
                assert np.array_equal(base.join_numpy(base.split_numpy(x, b, width, 100, op), b, width, 100, op), x), (kind, width, op, whole)
    x, b = bc.kernel_data("straddle", 8, 64, noise)
    assert list(x[:16].view("<u8")) == [(1 << 32) - 1, (1 << 32) + 1] and list(b[:16].view("<u8")) == [1 << 32, (1 << 32) - 2]


def test_a_span_between_superblock_borders_transforms_alone():
    rs = np.random.RandomState(3)
    x, b = rs.randint(0, 256, 5 * 800 + 61, dtype=np.uint8), rs.randint(0, 256, 5 * 800 + 61, dtype=np.uint8)
    for op in bc.OPS:
        y = base.split_numpy(x, b, 8, 100, op)
        for lo, hi in ((0, 800), (800, 2400), (1600, len(x)), (4000, len(x))):
            assert np.array_equal(base.split_numpy(x[lo:hi], b[lo:hi], 8, 100, op), y[lo:hi])
            assert np.array_equal(base.join_numpy(y[lo:hi], b[lo:hi], 8, 100, op), x[lo:hi])
    text = open(os.path.join(ROOT, "include", "rcx_base.h")).read()
    assert "SAME SPAN OF THE BASE" in text  # the header says so: range unpack depends on it


# ---- the kernel's unit arithmetic on the host, sanitized -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """tests/sim/base_sim.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer -> run(width, op, join, src, base)."""
    where = tmp_path_factory.mktemp("base_sim")
    exe = str(where / "base_sim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "base_sim.cpp")], check=True)

    def run(width, op, join, src, ref):
        (where / "src").write_bytes(src.tobytes())
        (where / "base").write_bytes(ref.tobytes())
        r = subprocess.run([exe, str(width), str(op), str(int(join)), str(where / "src"), str(where / "base"), str(where / "out")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and "base_sim ok" in r.stdout, (width, op, join, r.returncode, r.stdout + r.stderr)
        return np.frombuffer((where / "out").read_bytes(), np.uint8)

    return run


@pytest.mark.parametrize("width", bc.WIDTHS)
def test_unit_arithmetic_in_a_sanitized_program_is_the_twin(sim, width):
    """Every unit is a superblock at block = 16, so what a lane does with a unit -- the word arithmetic and the transpose -- is
    the twin's transform of those bytes; inside the program the scalar statement the rest lanes use must agree as well."""
    e, b = bc.edge_units(width)
    bits, flat_e, flat_b = 8 * width, e.reshape(-1), b.reshape(-1)
    values, bases = flat_e.view(f"<u{width}").astype(object), flat_b.view(f"<u{width}").astype(object)
    mask = (1 << bits) - 1
    differences = {(int(v) - int(w)) & mask for v, w in zip(values, bases)}
    assert {0, mask, 1, 1 << (bits - 1), (1 << (bits - 1)) - 1, ((1 << (bits - 1)) + 1) & mask} <= differences  # equal, base - 1, base + 1, the most negative
    if width == 8:
        assert any(int(v) < 1 << 32 <= int(w) for v, w in zip(values, bases)) and any(int(w) < 1 << 32 <= int(v) for v, w in zip(values, bases))
    for op in bc.OPS:
        want = base.split_numpy(flat_e, flat_b, width, 16, op)
        got = sim(width, op, False, flat_e, flat_b)
        assert np.array_equal(got, want), (width, op, np.flatnonzero(got != want)[:8])
        back = sim(width, op, True, want, flat_b)
        assert np.array_equal(back, flat_e), (width, op, np.flatnonzero(back != flat_e)[:8])
        # and the scalar loop in Python integers, so that the twin is not its own judge
        r = pc.join_numpy(want, width, 16).view(f"<u{width}") if width > 1 else want
        for k in range(0, len(values), 7):
            d = (int(values[k]) - int(bases[k])) & mask
            expect = int(values[k]) ^ int(bases[k]) if op == base.XOR else d if op == base.SUB else ((d << 1) ^ (0 - (d >> (bits - 1)))) & mask
            assert int(r[k]) == expect, (width, op, k)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_base.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, rcx, stats, stored, stored_items, typed_items
    build.build()
    names = declared_symbols()
    assert len(names) == 4 and set(names) == set(base.EXPORTS) == {"rcx_base_split_device", "rcx_base_join_device", "rcx_base_split", "rcx_base_join"}
    for name in names:
        assert getattr(base.lib(), name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "rcx_base.h")).read()
    assert '#include "rcx_planes.h"' in text
    for name, value in (("XOR", 0), ("SUB", 1), ("SUBZZ", 2)):
        assert getattr(base, name) == value and re.search(rf"#define RCX_BASE_{name} {value}u\b", text)
    # the other headers are what they were
    assert len(rcx.EXPORTS) == 57 and rcx.lib().rcx_version() == 300
    others = set(rcx.EXPORTS)
    for module in (planes, predict, stats, stored, stored_items, typed_items):
        others |= set(module.EXPORTS)
    assert not set(base.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_base.hpp", "rcx_base_api.hpp")) and any(h.endswith("rcx_base.h") for h in build.HEADERS)
    api = open(os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_api.hip")).read()
    assert '#include "rcx_base_api.hpp"' in api


def test_importing_the_container_stays_light():
    code = ("import sys; from cpprcoder_amd import container; "
            "assert 'torch' not in sys.modules and 'cpprcoder_amd.base' not in sys.modules and 'cpprcoder_amd.rcx' not in sys.modules; print('light')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "light" in r.stdout, r.stderr


# ---- RCXD --------------------------------------------------------------------------------------------------------------------
OFFS = np.array([0, 100, 250, 251], np.uint64)
N3 = 3 * 4096 - 7
BASE_CRCS = np.array([0xCBF43926, 0, 0xFFFFFFFF], np.uint32)


def inner_typed(width=4, pred=0, n=N3, block=4096, crcs=None):
    return container.typed_header_bytes(2, block, n, width, OFFS, crcs, pred=pred) + bytes(251)


def inner_blocks(flags=0, n=N3, block=4096, crcs=None):
    return container.header_bytes(2, block, n, OFFS, flags, crcs) + bytes(251)


def delta_blob(op=2, width=4, base_crcs=None, inner=None, n=N3, block=4096):
    return container.delta_header_bytes(op, width, block, n, base_crcs) + (inner if inner is not None else inner_blocks() if width == 1 else inner_typed(width))


def test_every_layout_name_is_a_name_of_the_container():
    for name in ("DELTA_MAGIC", "DELTA_VERSION", "BASE_OPS", "delta_header_bytes", "parse_delta", "BaseMismatchError"):
        assert getattr(container, name) is getattr(layout, name)
    assert container.DELTA_MAGIC == b"RCXD" and container.DELTA_VERSION == 1 and container.BASE_OPS == {"xor": 0, "sub": 1, "subzz": 2}
    assert issubclass(container.BaseMismatchError, container.ContainerError) and container.BaseMismatchError(7).index == 7
    assert "RCXD" in layout.__doc__ and "RCXD" in container.__doc__


def test_header_round_trips_for_both_inner_kinds():
    for width in (1, 2, 4, 8):
        for op in (0, 1, 2):
            for base_crcs in (None, BASE_CRCS):
                for crcs in (None, np.array([1, 2, 3], np.uint32)):
                    inner = inner_blocks(crcs=crcs) if width == 1 else inner_typed(width, crcs=crcs)
                    c = container.parse_delta(delta_blob(op, width, base_crcs, inner))
                    assert (c["op"], c["width"], c["block"], c["n"], c["kind"]) == (op, width, 4096, N3, "blocks" if width == 1 else "typed")
                    assert c["flags"] == (1 if base_crcs is not None else 0) and c["inner_at"] == 24 + (12 if base_crcs is not None else 0)
                    assert (c["base_crcs"] is None) if base_crcs is None else np.array_equal(c["base_crcs"], BASE_CRCS)
                    i = c["inner"]
                    assert (i["coder"], i["block"], i["n"], i["nblocks"]) == (2, 4096, N3, 3) and np.array_equal(i["offsets"], OFFS) and len(i["payload"]) == 251
                    assert (i["crcs"] is None) if crcs is None else np.array_equal(i["crcs"], crcs)
                    # an RCXT (RCXB) reader that skips the prefix gets the residual's container
                    skipped = delta_blob(op, width, base_crcs, inner)[c["inner_at"]:]
                    assert skipped == inner and (container.parse(skipped) if width == 1 else container.parse_typed(skipped))["n"] == N3
    # inner options: stored blocks
    offs = np.array([0, 4096, 4200, 4201], np.uint64)
    inner = container.typed_header_bytes(0, 4096, N3, 2, offs, None, 0, [1, 0, 0]) + bytes(4201)
    c = container.parse_delta(container.delta_header_bytes(1, 2, 4096, N3, BASE_CRCS) + inner)
    assert list(c["inner"]["stored"]) == [True, False, False]
    # nothing to code
    c = container.parse_delta(container.delta_header_bytes(0, 1, 65536, 0, np.zeros(0, np.uint32)) + container.header_bytes(0, 65536, 0, np.zeros(1, np.uint64)))
    assert c["n"] == 0 and len(c["base_crcs"]) == 0 and c["flags"] == 1


def test_layout_byte_for_byte():
    fixed = struct.pack("<4sBBBBI4sQ", b"RCXD", 1, 2, 4, 1, 4096, bytes(4), N3)
    assert len(fixed) == 24
    blob = delta_blob(2, 4, BASE_CRCS)
    assert blob == fixed + BASE_CRCS.astype("<u4").tobytes() + inner_typed(4)
    assert (blob[:4], blob[4], blob[5], blob[6], blob[7], blob[12:16]) == (b"RCXD", 1, 2, 4, 1, bytes(4))
    assert delta_blob(0, 1) == struct.pack("<4sBBBBI4sQ", b"RCXD", 1, 0, 1, 0, 4096, bytes(4), N3) + inner_blocks()
    text = layout.__doc__
    for line in ("0   4  magic  b\"RCXD\"", "5   1  op", "6   1  width", "7   1  flags", "8   4  block size", "12  4  zero", "16  8  n"):
        assert line in text, line


def test_refusals():
    def with_byte(b, at, value):
        out = bytearray(b)
        out[at] = value
        return bytes(out)

    good, guarded, narrow = delta_blob(2, 4), delta_blob(2, 4, BASE_CRCS), delta_blob(1, 1)
    for blob in (good, guarded, narrow):
        container.parse_delta(blob)
    bad = [with_byte(good, 4, 0), with_byte(good, 4, 2), with_byte(good, 5, 3), with_byte(good, 5, 255)]      # version, op
    bad += [with_byte(good, 6, w) for w in (0, 3, 5, 16)]                                                       # width
    bad += [with_byte(good, 7, f) for f in (2, 3, 4, 0x80)]                                                     # flags
    bad += [with_byte(good, at, 1) for at in range(12, 16)]                                                     # each reserved byte
    bad += [with_byte(good, 0, ord("X")), good[:23], good[:24], guarded[:30], good + b"x", good[:-1]]           # magic, truncation
    bad += [with_byte(good, 7, 1)]                                                                              # a table that is not there
    bad += [delta_blob(2, 4, inner=inner_blocks()), delta_blob(2, 1, inner=inner_typed(2)),                     # an inner container of the wrong magic
            delta_blob(2, 4, inner=container.item_header_bytes(0, [3], [0, 3]) + bytes(3)), delta_blob(2, 4, inner=good)]
    bad += [delta_blob(2, 4, inner=inner_typed(4, pred=1)), delta_blob(2, 4, inner=inner_typed(4, pred=2))]     # with a predictor
    sorted_n = N3  # coded_size(N3, blksort) = N3 (less than 32 KiB): the same table fits
    bad += [delta_blob(2, 1, inner=inner_blocks(container.FLAG_BLKSORT, n=sorted_n))]                           # with block sort
    bad += [delta_blob(2, 4, inner=inner_typed(8)), delta_blob(2, 4, inner=inner_typed(2))]                     # width disagrees
    bad += [delta_blob(2, 4, inner=inner_typed(4, n=N3 - 1)), delta_blob(2, 1, inner=inner_blocks(n=N3 - 1)),   # n disagrees
            delta_blob(2, 4, inner=inner_typed(4, block=4100)), with_byte(good, 9, 0x20)]  # block disagrees (both ways)
    for k, damaged in enumerate(bad):
        with pytest.raises(container.ContainerError):
            container.parse_delta(damaged)
            pytest.fail(f"case {k} parsed")
    # the writer refuses what the parser would
    for args in ((3, 4, 4096, N3), (-1, 4, 4096, N3), (True, 4, 4096, N3), ("sub", 4, 4096, N3), (1, 3, 4096, N3), (1, 0, 4096, N3), (1, 4, 15, N3),
                 (1, 4, (1 << 24), N3)):
        with pytest.raises(container.ContainerError):
            container.delta_header_bytes(*args)
    with pytest.raises(container.ContainerError):
        container.delta_header_bytes(1, 4, 4096, N3, BASE_CRCS[:2])  # one checksum per block of the base
    # the four other parsers refuse an RCXD blob as foreign, and parse_delta refuses theirs
    for parse in (container.parse, container.parse_items, container.parse_typed, container.parse_typed_items):
        for blob in (good, guarded, narrow):
            with pytest.raises(container.ContainerError):
                parse(blob)
    foreign = [inner_blocks(), inner_typed(4), container.item_header_bytes(0, [3], [0, 3]) + bytes(3),
               container.typed_items_header_bytes(0, [8], [4], [0], [0, 1, 2, 3, 4]) + bytes(4)]
    container.parse_typed_items(foreign[3])
    for blob in foreign:
        with pytest.raises(container.ContainerError):
            container.parse_delta(blob)


def test_what_pack_and_unpack_refuse_before_they_need_a_gpu():
    ints = np.arange(64, dtype=np.int64)
    for op in ("add", "zigzag", None, 2, b"sub", "SUB"):
        with pytest.raises(container.ContainerError):
            container.pack_delta(ints, ints, op=op)
    for data, ref, width in ((b"abcdefgh", b"abcdefgh", None), (b"abcdefgh", b"abcdefgh", 3), (ints, ints[:-1], None), (b"abcd", b"abc", 1),
                             (np.zeros(8, np.uint16), np.zeros(8, np.uint8), None), (ints, ints, 16)):
        with pytest.raises(container.ContainerError):
            container.pack_delta(data, ref, width)
    with pytest.raises(container.ContainerError):
        container.pack_delta(ints, ints, stored=1.5)
    # nothing to code: headers and no GPU, for both inner kinds
    for data, width, kind in ((np.zeros(0, np.int32), None, "typed"), (b"", 1, "blocks"), (np.zeros(0, np.uint8), None, "blocks")):
        for base_check in (True, False):
            blob = container.pack_delta(data, data, width, checksum=True, base_check=base_check)
            c = container.parse_delta(blob)
            assert (c["n"], c["kind"], c["op"]) == (0, kind, 2) and (c["base_crcs"] is not None) == base_check and c["inner"]["crcs"] is not None
            assert container.unpack_delta(blob, b"") == b"" and container.unpack_delta_range(blob, b"", 0, 0) == b""
            with pytest.raises(container.ContainerError):
                container.unpack_delta(blob, b"x")  # a base of another length
            with pytest.raises(container.ContainerError):
                container.unpack_delta_range(blob, b"", 0, 1)
    # a base of another length is refused before the GPU is looked for
    blob = delta_blob(2, 4, BASE_CRCS)
    for call in (lambda: container.unpack_delta(blob, bytes(N3 - 1)), lambda: container.unpack_delta_range(blob, bytes(N3 + 1), 0, 5),
                 lambda: container.unpack_delta_range(blob, bytes(N3), 5, N3 + 1)):
        with pytest.raises(container.ContainerError):
            call()


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_command_line_takes_a_base():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    a = ap.parse_args(["c", "--planes", "2", "--base", "old.bin", "--crc", "in", "out"])
    assert a.planes == 2 and a.base == "old.bin" and a.base_op is None and a.crc
    a = ap.parse_args(["c", "--base", "old.bin", "--stored", "--base-op", "xor", "in", "out"])
    assert a.planes is None and a.base_op == "xor" and a.stored is True
    assert ap.parse_args(["d", "--base", "old.bin", "in", "out"]).base == "old.bin" and ap.parse_args(["d", "in", "out"]).base is None
    assert ap.parse_args(["t", "--planes", "8", "--base", "old.bin", "--base-op", "sub", "f"]).base_op == "sub"
    assert ap.parse_args(["c", "in", "out"]).base is None and ap.parse_args(["t", "f"]).base is None
    for argv in (["c", "--blksort", "--base", "old.bin", "in", "out"], ["c", "--planes", "4", "--predict", "delta", "--base", "old.bin", "in", "out"],
                 ["t", "--blksort", "--base", "old.bin", "f"], ["t", "--planes", "4", "--predict", "auto", "--base", "old.bin", "f"],
                 ["c", "--base", "old.bin", "--base-op", "add", "in", "out"], ["c", "--base-op", "sub", "in", "out"], ["c", "--base", "in", "out"],
                 ["d", "--base-op", "sub", "--base", "old.bin", "in", "out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    import cpprcoder_amd.__main__ as cli
    assert "--base FILE" in cli.__doc__ and "RCXD" in cli.__doc__


# ---- why it exists, with the CPU oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint_sizes(oracle):
    """The oracle-coded sizes (adaptive coder, 64 KiB blocks) of w2's plain planes and of its residuals' split text, computed once."""
    w2, w, other = bc.checkpoint_pair()
    assert len(w2) == 2 << 20
    out = {"planes": pc.total_size(oracle, pc.split_numpy(w2, 2, 65536), 65536, 0)}
    for op in bc.OPS:
        out[bc.NAMES[op]] = pc.total_size(oracle, base.split_numpy(w2, w, 2, 65536, op), 65536, 0)
    out["unrelated"] = pc.total_size(oracle, base.split_numpy(w2, other, 2, 65536, base.SUBZZ), 65536, 0)
    return out


def test_a_checkpoint_codes_to_less_than_half_against_the_one_before(checkpoint_sizes):
    """1 Mi bf16 weights randn * 0.02 moved by randn * 1e-4: the subzz residual's split text codes to less than half of the plain
    planes (the order-0 estimate says 0.34); against an independent randn * 0.02 it codes to MORE than the plain planes."""
    s = checkpoint_sizes
    print(s, {k: round(v / s["planes"], 4) for k, v in s.items()})
    assert 2 * s["subzz"] < s["planes"]
    assert s["unrelated"] > s["planes"]


def test_the_sizes_the_readme_quotes(checkpoint_sizes, oracle):
    now, before = bc.counter_pair()
    counters = {"planes": pc.total_size(oracle, pc.split_numpy(now, 8, 65536), 65536, 0),
                "sub": pc.total_size(oracle, base.split_numpy(now, before, 8, 65536, base.SUB), 65536, 0)}
    print(checkpoint_sizes, counters)
    assert 2 * counters["sub"] < counters["planes"]
    assert checkpoint_sizes == README_BF16 and counters == README_COUNTERS


README_BF16 = {"planes": 1402412, "xor": 551423, "sub": 601164, "subzz": 481700, "unrelated": 1474187}
README_COUNTERS = {"planes": 658418, "sub": 97358}
