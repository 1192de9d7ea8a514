"""The device-planned base join as far as it goes without a GPU (include/rcx_base_picks.h): the numpy model of the planner
(base_picks.plan_numpy) on crafted tables with an entry of every kind, the latch order, the counts, the overflow rule, the
scratch formula, what the library and the binding refuse without a device, the header against base_picks.EXPORTS, and the
planner's rules (csrc/rcx_base_picks.hpp) in a sanitized program over the base item kernels' case list, held to the host plan."""
import os
import re
import subprocess

import numpy as np
import pytest

import base_items_cases as bc
from cpprcoder_amd import base_items, base_picks, build, container, picks, rcx, typed_picks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = base_picks.MAX_BLOCK
PAST = 1 << 63
NB = base_items.NO_BASE
SRC_CAP, BASE_CAP, DST_CAP = 10_000, 5_000, 20_000

# (src_at, base_at, dst_at, len, width, pred, op) -> what the entry is skipped with, None: it joins
CRAFTED = [
    ((0, PAST, 0, 100, 2, 0, NB), None),                 # no op: the base offset is not looked at
    ((100, PAST, 100, 33, 4, 1, NB), None),
    ((0, 0, 0, 100, 2, 0, 2), None),
    ((0, 0, 0, 100, 3, 0, 0), rcx.E_CORRUPT),
    ((0, 0, 0, 100, 0, 0, NB), rcx.E_CORRUPT),
    ((0, 0, 0, 100, 16, 0, 1), rcx.E_CORRUPT),
    ((0, 0, 0, 100, 2, 3, NB), rcx.E_CORRUPT),
    ((0, 0, 0, 100, 1, 1, NB), rcx.E_CORRUPT),           # a predictor on width 1
    ((0, 0, 0, 100, 4, 0, 3), rcx.E_CORRUPT),            # op 3
    ((0, 0, 0, 100, 4, 0, 254), rcx.E_CORRUPT),
    ((0, 0, 0, 100, 4, 1, 0), rcx.E_CORRUPT),            # a predictor and an op together
    ((0, 0, 0, 100, 8, 2, 2), rcx.E_CORRUPT),
    ((0, 0, 0, MB + 1, 1, 0, 0), rcx.E_CORRUPT),         # len / w + len % w one above RCX_MAX_BLOCK, before any cap is looked at
    ((0, 0, 0, 2 * MB + 1, 2, 0, 1), rcx.E_CORRUPT),
    ((PAST, PAST, PAST, 100, 4, 0, 3), rcx.E_CORRUPT),   # corrupt before capacity
    ((9_950, 0, 0, 100, 2, 0, 1), rcx.E_CAPACITY),       # the source past its cap
    ((9_900, 0, 0, 100, 2, 0, 1), None),                 # ... and exactly at it
    ((0, 0, 19_950, 100, 4, 0, 0), rcx.E_CAPACITY),      # the destination past its cap
    ((0, 0, 19_900, 100, 4, 0, 0), None),
    ((0, 4_901, 0, 100, 8, 0, 2), rcx.E_CAPACITY),       # the base span past its cap by one byte
    ((0, 4_900, 0, 100, 8, 0, 2), None),
    ((0, 4_901, 0, 100, 8, 0, NB), None),                # ... which nobody looks at without an op
    ((0, (1 << 64) - 10, 0, 100, 2, 0, 0), rcx.E_CAPACITY),  # a base position whose sum would wrap
    (((1 << 64) - 10, 0, 0, 100, 2, 0, NB), rcx.E_CAPACITY),
    ((PAST, PAST, PAST, 0, 77, 99, 55), None),           # length 0 with garbage beside it: not looked at
    ((0, 0, 0, 100, 2, 0, 2), None),                     # a repeat
]


def tables(entries):
    cols = list(zip(*[e for e, _ in entries])) if entries else [[]] * 7
    return tuple(np.array(cols[j], np.uint64) for j in range(4)) + tuple(np.array(cols[j], np.uint8) for j in range(4, 7))


def plan(entries, count, max_bytes=1 << 30):
    a, ba, b, n, w, p, o = tables(entries)
    return base_picks.plan_numpy(a, ba, b, n, w, p, o, count, max_bytes, SRC_CAP, BASE_CAP, DST_CAP)


def route_of(entry):
    return 0 if entry[3] == 0 else base_picks.BASE if entry[6] != NB else base_picks.SCAN if entry[5] else base_picks.ROWS


def test_every_kind_of_entry():
    """Each crafted entry alone between two good ones: it is skipped with its status at its position, or it joins by its route."""
    good = ((0, 0, 0, 64, 8, 0, 1), None)
    for entry, status in CRAFTED:
        m = plan([good, (entry, status), good], 3)
        if status is None:
            assert m["status"] == rcx.OK and m["position"] is None, entry
            assert bool(m["valid"][1]) == (entry[3] > 0) and m["route"][1] == route_of(entry), entry
        else:
            assert (m["status"], m["position"]) == (status, 1) and not m["valid"][1] and m["route"][1] == base_picks.NONE, entry
        assert m["valid"][0] and m["valid"][2] and m["route"][0] == m["route"][2] == base_picks.BASE
        assert m["bytes"] == 128 + (entry[3] if status is None else 0)


def test_one_entry_of_every_kind_in_its_class():
    """The 4 typed classes, the 3 predictors and the 12 base classes, one entry each of 16 units and a rest: each stands in its
    class of its set (or on the scan list), the heads count it, and the base set's workgroup step is RCX_BASE_ROWS(w) rows."""
    kinds = [(w, 0, NB) for w in bc.WIDTHS] + [(4, 1, NB), (8, 2, NB), (2, 1, NB)] + [(w, 0, op) for w in bc.WIDTHS for op in bc.OPS]
    assert len(kinds) == 19
    n = [16 * 16 * w + w + 1 for w, _, _ in kinds]
    at = np.cumsum([0] + n[:-1]).astype(np.uint64)
    m = base_picks.plan_numpy(at, at, at, n, [k[0] for k in kinds], [k[1] for k in kinds], [k[2] for k in kinds], 19, sum(n), sum(n), sum(n), sum(n))
    assert m["status"] == rcx.OK and list(m["route"]) == [1] * 4 + [2] * 3 + [3] * 12
    t, b = m["typed"], m["base"]
    assert list(np.diff(t["ent_first"].astype(int))) == [1, 0, 0] * 4 and list(t["entry"]) == [0, 1, 2, 3]
    assert list(np.diff(b["ent_first"].astype(int))) == [1] * 12 and list(b["entry"]) == list(range(7, 19))
    assert list(b["ufirst"]) == [16 * k for k in range(13)] and list(b["step_end"]) == list(range(1, 13)) and list(b["bat"]) == list(at[7:])
    assert list(np.diff(b["row_first"].astype(int))) == [2] * 12 and list(b["rowtab"]) == [k for k in range(12) for _ in (0, 1)]
    assert list(b["rest_end"]) == list(np.cumsum([1] * 12))
    # a class of 8 * 256 + 1 units of width 1 with an op is two steps of the base set, and one of the typed set without
    big = (8 * 256 + 1) * 16
    for op, name, steps in ((0, "base", 2), (NB, "typed", 1)):
        m = base_picks.plan_numpy([0], [0], [0], [big], [1], None, [op], 1, big, big, big, big)
        assert m[name]["step_end"][-1] == steps and m[name]["row_first"][-1] == 10


def test_latch_order_and_counts():
    """CORRUPT before CAPACITY, the lowest position of either; counts from 0 to above max_pick; entries behind the count hold anything."""
    m = plan(CRAFTED, len(CRAFTED))
    assert (m["status"], m["position"]) == (rcx.E_CORRUPT, 3) and m["valid"].sum() == sum(1 for e, s in CRAFTED if s is None and e[3])
    for count in range(len(CRAFTED) + 3):
        m = plan(CRAFTED, count)
        meant = min(count, len(CRAFTED))
        assert m["count"] == meant and not m["valid"][meant:].any() and not m["route"][meant:].any()
        bad = [k for k in range(meant) if CRAFTED[k][1] is not None] + ([len(CRAFTED)] if count > len(CRAFTED) else [])
        corrupt = any(CRAFTED[k][1] == rcx.E_CORRUPT for k in bad if k < len(CRAFTED))
        assert m["position"] == (min(bad) if bad else None) and m["status"] == (rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if bad else rcx.OK), count
        assert len(m["typed"]["entry"]) + len(m["base"]["entry"]) + (m["route"] == base_picks.SCAN).sum() == m["valid"].sum()
    # capacity alone (the base span), then a corrupt entry behind it: the status changes, the position stays the lowest
    three = [CRAFTED[19], CRAFTED[0], CRAFTED[8]]
    assert [(m["status"], m["position"]) for m in (plan(three, c) for c in (2, 3))] == [(rcx.E_CAPACITY, 0), (rcx.E_CORRUPT, 0)]


def test_overflow_rule():
    """The lengths of the entries that passed at max_bytes: all join; one above: nothing is joined, both sets are empty and
    RCX_E_CAPACITY stands at the count -- skipped entries and entries behind the count do not count."""
    total = sum(e[3] for e, s in CRAFTED if s is None)
    m = plan(CRAFTED, len(CRAFTED), total)
    assert m["bytes"] == total and not m["overflow"] and m["route"].any() and len(m["base"]["entry"]) > 0
    m = plan(CRAFTED, len(CRAFTED), total - 1)
    assert m["overflow"] and not m["route"].any() and m["valid"].any() and (m["status"], m["position"]) == (rcx.E_CORRUPT, 3)
    assert len(m["base"]["entry"]) == 0 and len(m["typed"]["entry"]) == 0 and m["base"]["step_end"][-1] == 0 and m["base"]["rest_end"][-1] == 0
    three = [CRAFTED[0], CRAFTED[2], CRAFTED[0]]
    m = plan(three, 2, 199)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 2, True)
    m = plan(three, 5, 299)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 3, True)  # min(count, max_pick), and the count's own latch
    assert not plan(three, 5, 300)["overflow"]


def test_without_ops_it_is_the_typed_model():
    """ops = None: status, position, routes and bins are typed_picks.plan_numpy's for the same tables."""
    a, ba, b, n, w, p, o = tables(CRAFTED)
    for count in (0, 5, len(CRAFTED), len(CRAFTED) + 1):
        for max_bytes in (1 << 30, 100):
            mine = base_picks.plan_numpy(a, None, b, n, w, p, None, count, max_bytes, SRC_CAP, 0, DST_CAP)
            theirs = typed_picks.plan_numpy(a, b, n, w, p, count, max_bytes, SRC_CAP, DST_CAP)
            for key in ("count", "bytes", "overflow", "status", "position"):
                assert mine[key] == theirs[key], (key, count, max_bytes)
            assert all(np.array_equal(mine[key], theirs[key]) for key in ("valid", "route", "bins")) and len(mine["base"]["entry"]) == 0


def test_scratch_formula():
    """The formula of the header is the library's answer, which needs no device; it holds the typed call's tables and more."""
    for max_pick in (1, 255, 256, 257, 1000, 200_000, base_picks.MAX_PICK):
        for max_bytes in (0, 1, 4095, 4096, 1 << 30, base_picks.MAX_BYTES):
            got = base_picks.scratch_bytes(max_pick, max_bytes)
            assert got == base_picks.scratch_formula(max_pick, max_bytes) and got % 8 == 0, (max_pick, max_bytes)
            assert got > typed_picks.scratch_bytes(max_pick, max_bytes)
    assert base_picks.scratch_bytes(0, 4096) == 0
    assert base_picks.scratch_bytes(base_picks.MAX_PICK + 1, 4096) == 0
    assert base_picks.scratch_bytes(10, base_picks.MAX_BYTES + 1) == 0
    assert base_picks.scratch_bytes(1000, 1 << 20) == 800 + 16 * 1001 + 56 * 1000 + 328 * 4 + 16 * 1000 + 4 * (256 + 8 + 256 + 24) + 8 * 5120 + 8 + 1000


def test_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "rcx_base_picks.h")).read()
    names = re.findall(r"^(?:int|uint64_t)\s+(rcx_\w+)\(", text, re.M)
    assert len(names) == 4 and set(names) == set(base_picks.EXPORTS), names
    lib = base_picks.lib()
    for name in names:
        getattr(lib, name)
    others = set(rcx.EXPORTS) | set(picks.EXPORTS) | set(typed_picks.EXPORTS) | set(base_items.EXPORTS)
    assert not set(base_picks.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_base_picks.hpp", "rcx_base_picks_api.hpp")) and any(h.endswith("rcx_base_picks.h") for h in build.HEADERS)
    source = open(os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_base_picks.hpp")).read()
    assert re.search(r"#define RCX_BPICK_KEYS 16u\b", source) and "rcx_base_picks_items_k" in source
    assert hasattr(container, "open_delta_items") and hasattr(container, "OpenDeltaItems")


def test_argument_errors_without_a_device():
    """RCX_E_ARG before anything is touched: no context; and the binding refuses tables that are not on the device, of the wrong
    element size, or too short, before it calls anything."""
    lib = base_picks.lib()
    assert lib.rcx_base_picks_reserve(None, 10, 100) == rcx.E_ARG
    assert lib.rcx_base_join_picks_device(None, None, 0, None, 0, None, None, None, None, None, None, None, None, 1, 16, None, 0, None) == rcx.E_ARG
    assert lib.rcx_base_join_picks(None, None, 0, None, 0, None, None, None, None, None, None, None, 0, None, 0) == rcx.E_ARG
    torch = pytest.importorskip("torch")

    class NoContext:
        _h = None

    t8, u8 = torch.zeros(4, dtype=torch.int64), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        base_picks.join_device(NoContext(), u8, u8, t8, t8, t8, t8, u8, None, u8, t8, u8, 64)
    meta = dict(device="meta")
    m8, mu = torch.zeros(4, dtype=torch.int64, **meta), torch.zeros(64, dtype=torch.uint8, **meta)

    class Cuda:  # stands where a cuda tensor stands, as far as the binding looks before it calls the library
        def __init__(self, t):
            self.t, self.is_cuda = t, True

        def __getattr__(self, name):
            return getattr(self.t, name)

    ok8, ok1 = Cuda(m8), Cuda(mu)
    with pytest.raises(ValueError, match="base_at holds contiguous 64-bit"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, Cuda(torch.zeros(4, dtype=torch.int32, **meta)), ok8, ok8, ok1, None, ok1, ok8, ok1, 64)
    with pytest.raises(ValueError, match="ops holds contiguous 8-bit"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, ok8, ok8, ok8, ok1, None, ok8, ok8, ok1, 64)
    with pytest.raises(ValueError, match="needs 5 entries"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, ok8, ok8, ok8, ok1, None, ok1, ok8, ok1, 64, max_pick=5)
    with pytest.raises(ValueError, match="base needs 65 entries"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, ok8, ok8, ok8, ok1, None, ok1, ok8, ok1, 64, base_cap=65)
    with pytest.raises(ValueError, match="max_bytes"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, ok8, ok8, ok8, ok1, None, ok1, ok8, ok1, base_picks.MAX_BYTES + 1)
    with pytest.raises(ValueError, match="max_pick"):
        base_picks.join_device(NoContext(), ok1, ok1, ok8, ok8, ok8, ok8, ok1, None, ok1, ok8, ok1, 64, max_pick=base_picks.MAX_PICK + 1)


def test_the_model_against_the_cases():
    """plan_numpy on a batch of every kind of item: every item is routed by its kind, and both sets' tables keep the caller's
    order within a class with ufirst an exact prefix sum."""
    case = next(c for c in bc.kernel_cases() if c["name"] == "mixed small")
    offs = bc.offsets_of(case)
    boffs, nbase = bc.base_layout(case)
    n, w, p, o = case["lengths"], case["widths"], case["preds"], case["ops"]
    total = int(n.sum())
    m = base_picks.plan_numpy(offs[:-1], boffs, offs[:-1], n, w, p, o, len(n), total, total, nbase, total)
    assert m["status"] == rcx.OK and m["bytes"] == total
    want = np.where(n == 0, 0, np.where(o != NB, base_picks.BASE, np.where(p != 0, base_picks.SCAN, base_picks.ROWS)))
    assert np.array_equal(m["route"], want)
    for name, second in (("typed", p), ("base", o)):
        s = m[name]
        e = s["entry"]
        cls = 3 * np.log2(w[e]).astype(int) + second[e]
        assert np.array_equal(cls, np.sort(cls)) and all(np.all(np.diff(e[cls == c]) > 0) for c in range(12))
        assert np.array_equal(np.diff(s["ufirst"].astype(np.int64)), (n[e].astype(np.int64) // w[e]) >> 4)
    assert np.array_equal(m["base"]["bat"], boffs[m["base"]["entry"]])


# ---- the rules, sanitized ------------------------------------------------------------------------------------------------------
def test_rules_in_a_sanitized_program(tmp_path):
    """tests/sim/base_picks_san.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: every batch of the base item kernels'
    case list, planned by the planner's plain functions in the planner's steps, gives rcx_base_items_plan's tables for the same
    items in the same order -- both heads, ufirst exact, every row -- and every unit is found in its own entry."""
    cases = bc.kernel_cases()
    exe, text = str(tmp_path / "base_picks_san"), str(tmp_path / "cases.txt")
    bc.write_cases(text, cases)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "base_picks_san.cpp")], check=True)
    r = subprocess.run([exe, text], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"base_picks_san ok: {len(cases)} batches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_residues_of_parity_cover_all_three_sides():
    """The GPU parity test's buffers: the packed sources at the batches' source offsets, the base spans in use at their base
    offsets and the scattered destinations at their destination offsets each stand at every residue mod 16."""
    import base_picks_cases as pc
    src, ref, dst = set(), set(), set()
    for c in bc.kernel_cases():
        t = pc.parity_tables(c)
        live = c["lengths"] > 0
        src |= {(int(o) + c["src_offset"]) % 16 for o in t["offs"][:-1][live]}
        ref |= {(int(o) + c["base_offset"]) % 16 for o in t["boffs"][live & (c["ops"] != NB)]}
        dst |= {(int(a) + c["dst_offset"]) % 16 for a in t["at"][live]}
    assert src == ref == dst == set(range(16))
