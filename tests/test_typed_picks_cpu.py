"""The device-planned typed join as far as it goes without a GPU (include/rcx_typed_picks.h): the numpy model of the planner
(typed_picks.plan_numpy) on crafted tables with an entry of every kind, the scratch formula, what the library and the binding
refuse without a device, the header against typed_picks.EXPORTS, and the planner's rules (csrc/rcx_typed_picks.hpp) in a
sanitized program over the typed item kernels' case list and the crafted bad entries, held to the model."""
import os
import re
import subprocess

import numpy as np
import pytest

import typed_items_cases as tc
from cpprcoder_amd import build, container, picks, rcx, typed_picks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = typed_picks.MAX_BLOCK
PAST = 1 << 63

# (src_at, dst_at, len, width, pred) with src_cap = 10_000 and dst_cap = 20_000 -> what the entry is skipped with, None: it joins
CRAFTED = [
    ((0, 0, 100, 2, 0), None),
    ((100, 100, 33, 4, 1), None),
    ((0, 0, 100, 3, 0), rcx.E_CORRUPT),
    ((0, 0, 100, 0, 0), rcx.E_CORRUPT),
    ((0, 0, 100, 5, 0), rcx.E_CORRUPT),
    ((0, 0, 100, 16, 0), rcx.E_CORRUPT),
    ((0, 0, 100, 255, 0), rcx.E_CORRUPT),
    ((0, 0, 100, 2, 3), rcx.E_CORRUPT),
    ((0, 0, 100, 8, 255), rcx.E_CORRUPT),
    ((0, 0, 100, 1, 1), rcx.E_CORRUPT),       # a predictor on width 1
    ((0, 0, 100, 1, 2), rcx.E_CORRUPT),
    ((0, 0, MB + 1, 1, 0), rcx.E_CORRUPT),    # len / w + len % w one above RCX_MAX_BLOCK, before any cap is looked at
    ((0, 0, 2 * MB + 1, 2, 0), rcx.E_CORRUPT),  # MB elements and one tail byte
    ((0, 0, 8 * (MB - 6) + 7, 8, 2), rcx.E_CORRUPT),
    ((9_950, 0, 100, 2, 0), rcx.E_CAPACITY),  # the source past its cap
    ((9_900, 0, 100, 2, 0), None),            # ... and exactly at it
    ((0, 19_950, 100, 4, 1), rcx.E_CAPACITY),  # the destination past its cap
    ((0, 19_900, 100, 4, 1), None),
    (((1 << 64) - 10, 0, 100, 2, 0), rcx.E_CAPACITY),  # a position whose sum would wrap
    ((0, (1 << 64) - 1, 2, 2, 0), rcx.E_CAPACITY),
    ((PAST, PAST, 0, 77, 99), None),          # length 0 with garbage beside it: not looked at
    ((0, 0, 100, 2, 0), None),                # a repeat of the first
    ((0, 0, 100, 2, 0), None),
]
SRC_CAP, DST_CAP = 10_000, 20_000


def tables(entries):
    cols = list(zip(*[e for e, _ in entries])) if entries else [[]] * 5
    return (np.array(cols[0], np.uint64), np.array(cols[1], np.uint64), np.array(cols[2], np.uint64), np.array(cols[3], np.uint8), np.array(cols[4], np.uint8))


def test_every_kind_of_entry():
    """Each crafted entry alone between two good ones: it is skipped with its status at its position, or it joins."""
    good = ((0, 0, 64, 8, 0), None)
    for entry, status in CRAFTED:
        a, b, n, w, p = tables([good, (entry, status), good])
        m = typed_picks.plan_numpy(a, b, n, w, p, 3, 1 << 30, SRC_CAP, DST_CAP)
        if status is None:
            assert m["status"] == rcx.OK and m["position"] is None, entry
            assert bool(m["valid"][1]) == (entry[2] > 0) and m["route"][1] == (0 if entry[2] == 0 else typed_picks.SCAN if entry[4] else typed_picks.ROWS)
        else:
            assert (m["status"], m["position"]) == (status, 1) and not m["valid"][1] and m["route"][1] == typed_picks.NONE, entry
        assert m["valid"][0] and m["valid"][2] and m["route"][0] == m["route"][2] == typed_picks.ROWS
        assert m["bytes"] == 128 + (entry[2] if status is None else 0)


def test_latch_order_and_counts():
    """CORRUPT before CAPACITY, the lowest position of either; counts from 0 to above max_pick; entries behind the count hold anything."""
    a, b, n, w, p = tables(CRAFTED)
    m = typed_picks.plan_numpy(a, b, n, w, p, len(CRAFTED), 1 << 30, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"]) == (rcx.E_CORRUPT, 2) and m["valid"].sum() == sum(1 for e, s in CRAFTED if s is None and e[2])
    for count in range(len(CRAFTED) + 3):
        m = typed_picks.plan_numpy(a, b, n, w, p, count, 1 << 30, SRC_CAP, DST_CAP)
        meant = min(count, len(CRAFTED))
        assert m["count"] == meant and not m["valid"][meant:].any() and not m["route"][meant:].any()
        bad = [k for k in range(meant) if CRAFTED[k][1] is not None] + ([len(CRAFTED)] if count > len(CRAFTED) else [])
        corrupt = any(CRAFTED[k][1] == rcx.E_CORRUPT for k in bad if k < len(CRAFTED))
        assert m["position"] == (min(bad) if bad else None) and m["status"] == (rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if bad else rcx.OK), count
    # capacity alone, then a corrupt entry behind it: the status changes, the position stays the lowest
    a, b, n, w, p = tables([CRAFTED[14], CRAFTED[0], CRAFTED[2]])
    assert [(m["status"], m["position"]) for m in (typed_picks.plan_numpy(a, b, n, w, p, c, 1 << 30, SRC_CAP, DST_CAP) for c in (2, 3))] == [
        (rcx.E_CAPACITY, 0), (rcx.E_CORRUPT, 0)]


def test_overflow_rule():
    """The lengths of the entries that passed at max_bytes: all join; one above: nothing is joined, RCX_E_CAPACITY at the count --
    skipped entries and entries behind the count do not count."""
    a, b, n, w, p = tables(CRAFTED)
    total = sum(e[2] for e, s in CRAFTED if s is None)
    m = typed_picks.plan_numpy(a, b, n, w, p, len(CRAFTED), total, SRC_CAP, DST_CAP)
    assert m["bytes"] == total and not m["overflow"] and m["route"].any()
    m = typed_picks.plan_numpy(a, b, n, w, p, len(CRAFTED), total - 1, SRC_CAP, DST_CAP)
    assert m["overflow"] and not m["route"].any() and m["valid"].any() and (m["status"], m["position"]) == (rcx.E_CORRUPT, 2)
    a, b, n, w, p = tables([CRAFTED[0], CRAFTED[1], CRAFTED[0]])
    m = typed_picks.plan_numpy(a, b, n, w, p, 2, 132, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 2, True)
    m = typed_picks.plan_numpy(a, b, n, w, p, 5, 232, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 3, True)  # min(count, max_pick), and the count's own latch


def test_bins():
    """Ascending bins are descending lengths: exact below 512, the leading one and eight bits above; the last length has the first bin."""
    assert typed_picks.BINS == 5120 and typed_picks.bin_of(1) == typed_picks.BINS - 2 and typed_picks.bin_of((1 << 27) - 1) == 0
    lengths = [1, 2, 511, 512, 513, 514, 1023, 1024, 1 << 20, (1 << 24) - 256, 8 * MB + 7]
    bins = [typed_picks.bin_of(n) for n in lengths]
    assert all(x >= y for x, y in zip(bins, bins[1:])) and bins[3] == bins[4] and bins[4] > bins[5] and len(set(bins[:3])) == 3
    for n in (0, 1 << 27):
        with pytest.raises(ValueError):
            typed_picks.bin_of(n)


def test_scratch_formula():
    """The formula of the header is the library's answer, which needs no device."""
    for max_pick in (1, 255, 256, 257, 1000, 200_000, typed_picks.MAX_PICK):
        for max_bytes in (0, 1, 4095, 4096, 1 << 30, typed_picks.MAX_BYTES):
            got = typed_picks.scratch_bytes(max_pick, max_bytes)
            assert got == typed_picks.scratch_formula(max_pick, max_bytes) and got % 8 == 0 and got > 53 * max_pick, (max_pick, max_bytes)
    assert typed_picks.scratch_bytes(0, 4096) == 0
    assert typed_picks.scratch_bytes(typed_picks.MAX_PICK + 1, 4096) == 0
    assert typed_picks.scratch_bytes(10, typed_picks.MAX_BYTES + 1) == 0
    assert typed_picks.scratch_bytes(1000, 1 << 20) == 400 + 8 * 1001 + 32 * 1000 + 88 * 4 + 12 * 1000 + 4 * (256 + 8) + 8 * 5120 + 8 + 1000


def test_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "rcx_typed_picks.h")).read()
    names = re.findall(r"^(?:int|uint64_t)\s+(rcx_\w+)\(", text, re.M)
    assert len(names) == 4 and set(names) == set(typed_picks.EXPORTS), names
    lib = typed_picks.lib()
    for name in names:
        getattr(lib, name)
    others = set(rcx.EXPORTS) | set(picks.EXPORTS)
    assert not set(typed_picks.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_typed_picks.hpp", "rcx_typed_picks_api.hpp")) and any(h.endswith("rcx_typed_picks.h") for h in build.HEADERS)
    assert (typed_picks.PLAN_THREADS, typed_picks.PLAN_GRID, typed_picks.PLAN_TOP) == (256, 512, 1024)
    source = open(os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_typed_picks.hpp")).read()
    for name, value in (("RCX_TPICK_THREADS", typed_picks.PLAN_THREADS), ("RCX_TPICK_GRID", typed_picks.PLAN_GRID), ("RCX_TPICK_TOP", typed_picks.PLAN_TOP),
                        ("RCX_TPICK_EXACT", typed_picks.EXACT)):
        assert re.search(rf"#define {name} {value}u\b", source), name


def test_argument_errors_without_a_device():
    """RCX_E_ARG before anything is touched: no context; and the binding refuses tables that are not on the device, of the wrong
    element size, or too short, before it calls anything."""
    lib = typed_picks.lib()
    assert lib.rcx_typed_picks_reserve(None, 10, 100) == rcx.E_ARG
    assert lib.rcx_typed_join_picks_device(None, None, 0, None, None, None, None, None, None, 1, 16, None, 0, None) == rcx.E_ARG
    assert lib.rcx_typed_join_picks(None, None, 0, None, None, None, None, None, 0, None, 0) == rcx.E_ARG
    torch = pytest.importorskip("torch")

    class NoContext:
        _h = None

    t8, t4 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        typed_picks.join_device(NoContext(), u8, t8, t8, t8, u8, None, t8, u8, 64)
    meta = dict(device="meta")
    m8, mu = torch.zeros(4, dtype=torch.int64, **meta), torch.zeros(64, dtype=torch.uint8, **meta)

    class Cuda:  # stands where a cuda tensor stands, as far as the binding looks before it calls the library
        def __init__(self, t):
            self.t, self.is_cuda = t, True

        def __getattr__(self, name):
            return getattr(self.t, name)

    ok8, ok1 = Cuda(m8), Cuda(mu)
    with pytest.raises(ValueError, match="64-bit"):
        typed_picks.join_device(NoContext(), ok1, Cuda(torch.zeros(4, dtype=torch.int32, **meta)), ok8, ok8, ok1, None, ok8, ok1, 64)
    with pytest.raises(ValueError, match="8-bit"):
        typed_picks.join_device(NoContext(), ok1, ok8, ok8, ok8, ok8, None, ok8, ok1, 64)
    with pytest.raises(ValueError, match="needs 5 entries"):
        typed_picks.join_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, 64, max_pick=5)
    with pytest.raises(ValueError, match="max_bytes"):
        typed_picks.join_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, typed_picks.MAX_BYTES + 1)
    with pytest.raises(ValueError, match="max_pick"):
        typed_picks.join_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, 64, max_pick=typed_picks.MAX_PICK + 1)
    assert t4.element_size() == 4 and hasattr(container, "open_typed_items")


# ---- the rules, sanitized ------------------------------------------------------------------------------------------------------
def write_batches(path, batches):
    """Per batch `n count max_bytes src_cap dst_cap status position`, then per entry `src_at dst_at len width pred route bin`, the
    last two and the batch's status and position from plan_numpy."""
    code = {rcx.OK: 0, rcx.E_CAPACITY: 1, rcx.E_CORRUPT: 2}
    with open(path, "w") as f:
        f.write(f"{len(batches)}\n")
        for a, b, n, w, p, count, max_bytes, src_cap, dst_cap in batches:
            m = typed_picks.plan_numpy(a, b, n, w, p, count, max_bytes, src_cap, dst_cap)
            f.write(f"{len(n)} {count} {max_bytes} {src_cap} {dst_cap} {code[m['status']]} {-1 if m['position'] is None else m['position']}\n")
            for k in range(len(n)):
                f.write(f"{int(a[k])} {int(b[k])} {int(n[k])} {int(w[k])} {int(p[k])} {int(m['route'][k])} {int(m['bins'][k])}\n")


def test_rules_in_a_sanitized_program(tmp_path):
    """tests/sim/typed_picks_san.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: the 25 batches of the typed item
    kernels' case list, shuffled, with scattered destinations; the crafted entries among good ones, at every count around a tile;
    a batch at max_bytes and one byte above; counts above max_pick.  The program agrees with plan_numpy and the plan keeps its
    invariants."""
    batches = []
    rs = np.random.RandomState(12)
    for case in tc.kernel_cases():
        n = case["lengths"].astype(np.uint64)
        order = rs.permutation(len(n))
        a = tc.offsets_of(case)[:-1][order]
        n, w, p = n[order], case["widths"][order], case["preds"][order]
        b = (np.cumsum(n + np.uint64(19)) - n).astype(np.uint64)
        total = int(n.sum())
        batches.append((a, b, n, w, p, len(n), total, total, total + 19 * len(n) + 19))
    assert len(batches) == 25
    good = tc.kernel_cases()[10]  # mixed small
    ga = tc.offsets_of(good)[:-1]
    gn, gw, gp = good["lengths"].astype(np.uint64), good["widths"], good["preds"]
    ca, cb, cn, cw, cp = tables(CRAFTED)
    for at in (0, 255, 256, 600):
        a, b, n, w, p = (np.concatenate([g[:at], c, g[at:]]) for g, c in ((ga, ca), (ga, cb), (gn, cn), (gw, cw), (gp, cp)))
        for count in (at, at + 3, len(n), len(n) + 1):
            batches.append((a, b, n, w, p, count, 1 << 30, SRC_CAP, DST_CAP))
    total = int(gn.sum())
    for max_bytes in (total, total - 1):
        batches.append((ga, ga, gn, gw, gp, len(gn), max_bytes, total, total))
    exe, cases = str(tmp_path / "typed_picks_san"), str(tmp_path / "batches.txt")
    write_batches(cases, batches)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "typed_picks_san.cpp")], check=True)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"typed_picks_san ok: {len(batches)} batches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
