"""The device-planned typed split as far as it goes without a GPU (include/rcx_typed_split_picks.h): the numpy model of the
planner (typed_split_picks.plan_numpy) on crafted tables with an entry of every kind, kept in every case, head and ufirst against
a numpy rendering of rcx_typed_plan(scan = false), the scratch formula, what the library and the binding refuse without a device,
the header against typed_split_picks.EXPORTS, PackedTypedItems.to_bytes' compaction against layout.parse_typed_items, and the
planner's rules (csrc/rcx_typed_split_picks.hpp) in a sanitized program over the typed item kernels' case list and the crafted bad
entries, held to the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import typed_items_cases as tc
from cpprcoder_amd import base_picks, build, container, encode_picks, layout, picks, rcx, typed_picks
from cpprcoder_amd import typed_split_picks as tsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = tsp.MAX_BLOCK
PAST = 1 << 63

# (src_at, dst_at, len, width, pred) with src_cap = 10_000 and dst_cap = 20_000 -> what the entry is skipped with, None: it is split
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
    ((10_001, 0, 1, 1, 0), rcx.E_CAPACITY),   # a source position past its cap
    ((0, 19_950, 100, 4, 1), rcx.E_CAPACITY),  # the destination past its cap
    ((0, 19_900, 100, 4, 1), None),
    (((1 << 64) - 10, 0, 100, 2, 0), rcx.E_CAPACITY),  # a position whose sum would wrap
    ((0, (1 << 64) - 1, 2, 2, 0), rcx.E_CAPACITY),
    ((PAST, PAST, 0, 77, 99), None),          # length 0 with garbage beside it: not looked at
    ((0, 0, 100, 2, 0), None),                # a repeat of the first
    ((0, 0, 64, 8, 2), None),
    ((0, 0, 7, 8, 1), None),                  # below one element: all tail
]
SRC_CAP, DST_CAP = 10_000, 20_000


def tables(entries):
    cols = list(zip(*[e for e, _ in entries])) if entries else [[]] * 5
    return (np.array(cols[0], np.uint64), np.array(cols[1], np.uint64), np.array(cols[2], np.uint64), np.array(cols[3], np.uint8), np.array(cols[4], np.uint8))


def host_plan(lengths, widths, preds):
    """rcx_typed_plan(..., scan = false) of csrc/rcx_typed_items.hpp, rendered in numpy for items given in the caller's order ->
    (the head as typed_split_picks.head_numpy returns it, ufirst uint64[nent + 1], the item at every entry)."""
    nc = tsp.CLASSES
    nent, units = [0] * nc, [0] * nc
    live = [i for i in range(len(lengths)) if int(lengths[i])]
    for i in live:
        c = tsp.class_of(widths[i], preds[i])
        nent[c] += 1
        units[c] += (int(lengths[i]) // int(widths[i])) >> 4
    step_end, rest_end, ubase, ent_first, row_first = [], [], [], [], []
    ents = rows = ub = steps = rests = 0
    for c in range(nc):
        w = 1 << (c // 3)
        ent_first.append(ents), row_first.append(rows), ubase.append(ub)
        step = 16 // w * 256
        steps += (units[c] + step - 1) // step
        rests += (nent[c] * 17 * w + 255) // 256
        step_end.append(steps), rest_end.append(rests)
        ents += nent[c]
        ub += units[c]
        if nent[c]:
            rows += (units[c] + 255) // 256 + 1
    head = {"step_end": step_end, "rest_end": rest_end, "ubase": ubase + [ub], "ent_first": ent_first + [ents], "row_first": row_first + [rows]}
    nxt, unit = list(ent_first), list(ubase)
    ufirst, item = np.zeros(ents + 1, np.uint64), np.zeros(ents, np.int64)
    for i in live:
        c = tsp.class_of(widths[i], preds[i])
        k = nxt[c]
        nxt[c] += 1
        ufirst[k], item[k] = unit[c], i
        unit[c] += (int(lengths[i]) // int(widths[i])) >> 4
    ufirst[ents] = ub
    return head, ufirst, item


def test_every_kind_of_entry():
    """Each crafted entry alone between two good ones: it is skipped with its status at its position and kept 0, or it is split
    and kept is its length."""
    good = ((0, 0, 64, 8, 0), None)
    for entry, status in CRAFTED:
        a, b, n, w, p = tables([good, (entry, status), good])
        m = tsp.plan_numpy(a, b, n, w, p, 3, 1 << 30, SRC_CAP, DST_CAP)
        if status is None:
            assert m["status"] == rcx.OK and m["position"] is None, entry
            assert bool(m["valid"][1]) == (entry[2] > 0) and m["kept"][1] == entry[2]
            assert m["klass"][1] == (tsp.NO_CLASS if entry[2] == 0 else tsp.class_of(entry[3], entry[4]))
        else:
            assert (m["status"], m["position"]) == (status, 1) and not m["valid"][1] and m["klass"][1] == tsp.NO_CLASS and m["place"][1] == -1, entry
            assert m["kept"][1] == 0
        assert m["valid"][0] and m["valid"][2] and m["klass"][0] == m["klass"][2] == 9 and list(m["kept"][[0, 2]]) == [64, 64]
        assert m["place"][0] < m["place"][2]  # the caller's order within the class
        assert m["bytes"] == 128 + (entry[2] if status is None else 0)


def test_latch_order_counts_and_kept():
    """CORRUPT before CAPACITY, the lowest position of either; counts from 0 to above max_pick; entries behind the count hold
    anything and have kept 0."""
    a, b, n, w, p = tables(CRAFTED)
    m = tsp.plan_numpy(a, b, n, w, p, len(CRAFTED), 1 << 30, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"]) == (rcx.E_CORRUPT, 2) and m["valid"].sum() == sum(1 for e, s in CRAFTED if s is None and e[2])
    for count in range(len(CRAFTED) + 3):
        m = tsp.plan_numpy(a, b, n, w, p, count, 1 << 30, SRC_CAP, DST_CAP)
        meant = min(count, len(CRAFTED))
        assert m["count"] == meant and not m["valid"][meant:].any() and not m["kept"][meant:].any() and (m["place"][meant:] == -1).all()
        bad = [k for k in range(meant) if CRAFTED[k][1] is not None] + ([len(CRAFTED)] if count > len(CRAFTED) else [])
        corrupt = any(CRAFTED[k][1] == rcx.E_CORRUPT for k in bad if k < len(CRAFTED))
        assert m["position"] == (min(bad) if bad else None) and m["status"] == (rcx.E_CORRUPT if corrupt else rcx.E_CAPACITY if bad else rcx.OK), count
        want = [CRAFTED[k][0][2] if k < meant and CRAFTED[k][1] is None else 0 for k in range(len(CRAFTED))]
        assert [int(x) for x in m["kept"]] == want, count
        assert sorted(m["place"][m["place"] >= 0]) == list(range(int(m["valid"].sum()))) and len(m["ufirst"]) == int(m["valid"].sum()) + 1
    # capacity alone, then a corrupt entry behind it: the status changes, the position stays the lowest
    a, b, n, w, p = tables([CRAFTED[14], CRAFTED[0], CRAFTED[2]])
    assert [(m["status"], m["position"]) for m in (tsp.plan_numpy(a, b, n, w, p, c, 1 << 30, SRC_CAP, DST_CAP) for c in (2, 3))] == [
        (rcx.E_CAPACITY, 0), (rcx.E_CORRUPT, 0)]


def test_overflow_rule():
    """The lengths of the entries that passed at max_bytes: all are split; one above: nothing is split, kept is all 0 and
    RCX_E_CAPACITY is latched at the count -- skipped entries and entries behind the count do not count."""
    a, b, n, w, p = tables(CRAFTED)
    total = sum(e[2] for e, s in CRAFTED if s is None)
    m = tsp.plan_numpy(a, b, n, w, p, len(CRAFTED), total, SRC_CAP, DST_CAP)
    assert m["bytes"] == total and not m["overflow"] and int(m["kept"].sum()) == total
    m = tsp.plan_numpy(a, b, n, w, p, len(CRAFTED), total - 1, SRC_CAP, DST_CAP)
    assert m["overflow"] and not m["kept"].any() and (m["place"] == -1).all() and m["valid"].any() and (m["status"], m["position"]) == (rcx.E_CORRUPT, 2)
    assert m["head"]["step_end"][-1] == m["head"]["rest_end"][-1] == m["head"]["ent_first"][-1] == 0 and list(m["ufirst"]) == [0]
    a, b, n, w, p = tables([CRAFTED[0], CRAFTED[1], CRAFTED[0]])
    m = tsp.plan_numpy(a, b, n, w, p, 2, 132, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 2, True) and not m["kept"].any()
    m = tsp.plan_numpy(a, b, n, w, p, 2, 133, SRC_CAP, DST_CAP)
    assert (m["status"], m["overflow"]) == (rcx.OK, False) and list(m["kept"]) == [100, 33, 0]
    m = tsp.plan_numpy(a, b, n, w, p, 5, 232, SRC_CAP, DST_CAP)
    assert (m["status"], m["position"], m["overflow"]) == (rcx.E_CAPACITY, 3, True)  # min(count, max_pick), and the count's own latch


@pytest.mark.parametrize("case", tc.kernel_cases(), ids=[c["name"] for c in tc.kernel_cases()])
def test_head_and_ufirst_are_the_host_plans(case):
    """The 25 batches of the typed item kernels: head, ufirst and the order of the entries are rcx_typed_plan(scan = false)'s."""
    n, w, p = case["lengths"], case["widths"], case["preds"]
    offs = tc.offsets_of(case)
    total = int(n.sum())
    m = tsp.plan_numpy(offs[:-1], offs[:-1], n, w, p, len(n), total, total, total)
    head, ufirst, item = host_plan(n, w, p)
    assert m["status"] == rcx.OK and m["head"] == head
    assert np.array_equal(m["ufirst"], ufirst) and np.array_equal(m["order"], item)
    assert np.array_equal(m["kept"], n) and head["row_first"][-1] <= total // 4096 + 24


def test_scratch_formula():
    """The formula of the header is the library's answer, which needs no device, and it is linear in both arguments."""
    for max_pick in (1, 255, 256, 257, 1000, 200_000, tsp.MAX_PICK):
        for max_bytes in (0, 1, 4095, 4096, 1 << 30, tsp.MAX_BYTES):
            got = tsp.scratch_bytes(max_pick, max_bytes)
            assert got == tsp.scratch_formula(max_pick, max_bytes) and got % 8 == 0 and got > 32 * max_pick, (max_pick, max_bytes)
    assert tsp.scratch_bytes(0, 4096) == 0
    assert tsp.scratch_bytes(tsp.MAX_PICK + 1, 4096) == 0
    assert tsp.scratch_bytes(10, tsp.MAX_BYTES + 1) == 0
    assert tsp.scratch_bytes(1000, 1 << 20) == 400 + 8 * 1001 + 16 * 1000 + 248 * 4 + 8 * 1000 + 4 * (256 + 24) + 8
    f = tsp.scratch_formula
    base = f(256, 8192)
    for k in (1, 2, 5, 1000):  # whole tiles and whole pairs of rows: the steps are equal
        assert f(256 * (k + 1), 8192) - f(256 * k, 8192) == f(512, 8192) - base == 256 * 32 + 248
        assert f(256, 8192 * (k + 1)) - f(256, 8192 * k) == f(256, 16384) - base == 8
    assert f(512, 16384) - base == (f(512, 8192) - base) + (f(256, 16384) - base)


def test_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "rcx_typed_split_picks.h")).read()
    names = re.findall(r"^(?:int|uint64_t)\s+(rcx_\w+)\(", text, re.M)
    assert len(names) == 4 and set(names) == set(tsp.EXPORTS), names
    lib = tsp.lib()
    for name in names:
        getattr(lib, name)
    assert len(rcx.EXPORTS) == 57
    others = set(rcx.EXPORTS) | set(picks.EXPORTS) | set(typed_picks.EXPORTS) | set(base_picks.EXPORTS) | set(encode_picks.EXPORTS)
    assert not set(tsp.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_typed_split_picks.hpp", "rcx_typed_split_picks_api.hpp"))
    assert any(h.endswith("rcx_typed_split_picks.h") for h in build.HEADERS)
    assert (tsp.PLAN_THREADS, tsp.PLAN_GRID, tsp.PLAN_TOP) == (typed_picks.PLAN_THREADS, typed_picks.PLAN_GRID, typed_picks.PLAN_TOP) == (256, 512, 1024)
    csrc = os.path.join(ROOT, "cpprcoder_amd", "csrc")
    source = open(os.path.join(csrc, "rcx_typed_split_picks.hpp")).read()
    assert "rcx_tpick_validate(" in source and "RCX_HD u32 rcx_tpick_validate" not in source  # the rule is reused, not copied
    every = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip")))
    for rule in ("u32 rcx_tpick_validate(", "void rcx_class_head(", "u32 rcx_len_bin("):  # one definition of each in csrc/
        assert every.count(rule) == 1, rule
    assert "_head(const u64*" not in every.replace("rcx_class_head(const u64*", "")  # and no second head under another name
    api = open(os.path.join(csrc, "rcx_typed_split_picks_api.hpp")).read()
    assert "hipMemset" not in api and "_clear_k" not in api  # kernel nodes alone, and no clear launch of its own;
    assert re.search(r"SCAN = false\b", source)  # the shared launches clear for a policy with a scan list only, and the split has none
    shared = open(os.path.join(csrc, "rcx_typed_picks_api.hpp")).read()
    assert shared.count("_clear_k") == 1 and "if (P::SCAN) hipLaunchKernelGGL(rcx_class_clear_k" in shared and "hipMemset" not in shared
    assert hasattr(container, "pack_typed_items_device") and container.PackedTypedItems is tsp.PackedTypedItems
    assert issubclass(tsp.PackedTypedItems, container.OpenTypedItems) and "_expand" not in vars(tsp.PackedTypedItems)


def test_argument_errors_without_a_device():
    """RCX_E_ARG before anything is touched: no context, each pointer null in turn, sizes above their bounds, overlapping ranges;
    and the binding refuses tables that are not on the device, of the wrong element size, or too short, before it calls anything."""
    lib = tsp.lib()
    assert lib.rcx_typed_split_picks_reserve(None, 10, 100) == rcx.E_ARG
    assert lib.rcx_typed_split_picks_device(None, None, 0, None, None, None, None, None, None, 1, 16, None, 0, None, None) == rcx.E_ARG
    assert lib.rcx_typed_split_picks(None, None, 0, None, None, None, None, None, 0, None, 0, None) == rcx.E_ARG
    # a context that is never looked into: every refusal below comes before the device is entered
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    mem = C.create_string_buffer(4096)
    at = C.addressof(mem)
    src, dst = at, at + 2048
    good = [src, 1024, at, at, at, at, at, at, 4, 1024, dst, 1024, at, None]  # src, cap, src_at, dst_at, len, widths, preds, count, max_pick, max_bytes, dst, cap, kept, stream
    for null in (0, 2, 3, 4, 5, 7, 10):  # each pointer in turn, d_preds (6) and d_kept (12) apart
        args = list(good)
        args[null] = None
        assert lib.rcx_typed_split_picks_device(ctx, *args) == rcx.E_ARG, null
    for at_, value in ((8, 1 << 31), (9, (1 << 42) + 1)):
        args = list(good)
        args[at_] = value
        assert lib.rcx_typed_split_picks_device(ctx, *args) == rcx.E_ARG, at_
        assert lib.rcx_typed_split_picks_reserve(ctx, *((value, 16) if at_ == 8 else (16, value))) == rcx.E_ARG
    for s, sc, d, dc in ((at, 1024, at + 1023, 1024), (at + 100, 1024, at, 101), (at, 2048, at + 512, 16), (at + 512, 16, at, 2048)):
        args = list(good)
        args[0], args[1], args[10], args[11] = s, sc, d, dc
        assert lib.rcx_typed_split_picks_device(ctx, *args) == rcx.E_ARG, (s - at, sc, d - at, dc)
    assert lib.rcx_typed_split_picks(ctx, src, 1024, at, at, at, at, None, 1 << 31, dst, 1024, None) == rcx.E_ARG
    assert lib.rcx_typed_split_picks(ctx, src, 1024, at, at, at, at, None, 4, src + 1023, 1024, None) == rcx.E_ARG
    assert lib.rcx_typed_split_picks(ctx, src, 1024, None, at, at, at, None, 4, dst, 1024, None) == rcx.E_ARG
    torch = pytest.importorskip("torch")

    class NoContext:
        _h = None

    t8 = torch.zeros(4, dtype=torch.int64)
    u8 = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda"):
        tsp.split_device(NoContext(), u8, t8, t8, t8, u8, None, t8, u8, 64)
    with pytest.raises(ValueError, match="cuda"):
        tsp.pack_typed_items_device(NoContext(), u8, t8, t8, u8, u8, t8, 4, 16, 64)
    meta = dict(device="meta")
    m8, mu = torch.zeros(4, dtype=torch.int64, **meta), torch.zeros(64, dtype=torch.uint8, **meta)

    class Cuda:  # stands where a cuda tensor stands, as far as the binding looks before it calls the library
        def __init__(self, t):
            self.t, self.is_cuda = t, True

        def __getattr__(self, name):
            return getattr(self.t, name)

    ok8, ok1 = Cuda(m8), Cuda(mu)
    with pytest.raises(ValueError, match="64-bit"):
        tsp.split_device(NoContext(), ok1, Cuda(torch.zeros(4, dtype=torch.int32, **meta)), ok8, ok8, ok1, None, ok8, ok1, 64)
    with pytest.raises(ValueError, match="8-bit"):
        tsp.split_device(NoContext(), ok1, ok8, ok8, ok8, ok8, None, ok8, ok1, 64)
    with pytest.raises(ValueError, match="needs 5 entries"):
        tsp.split_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, 64, max_pick=5)
    with pytest.raises(ValueError, match="kept needs 4 entries"):
        tsp.split_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, 64, kept=Cuda(torch.zeros(3, dtype=torch.int64, **meta)))
    with pytest.raises(ValueError, match="max_bytes"):
        tsp.split_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, tsp.MAX_BYTES + 1)
    with pytest.raises(ValueError, match="max_pick"):
        tsp.split_device(NoContext(), ok1, ok8, ok8, ok8, ok1, None, ok8, ok1, 64, max_pick=tsp.MAX_PICK + 1)
    with pytest.raises(ValueError, match="d_widths needs 4 entries"):
        tsp.pack_typed_items_device(NoContext(), ok1, ok8, ok8, Cuda(torch.zeros(3, dtype=torch.uint8, **meta)), ok1, ok8, 4, 16, 64)


def test_compaction_of_the_slots():
    """PackedTypedItems.to_bytes' compaction on fabricated tables: 8 slots an item, the slots behind the width empty -> the
    container's sub-item table; the container made from it parses (layout.parse_typed_items) to the items, the streams' sizes in
    sub-item order and the payload untouched."""
    rs = np.random.RandomState(8)
    classes = [(w, p) for w in tc.WIDTHS for p in tc.preds_of(w)]
    lengths = np.array([0, 1, 7, 16, 65, 300, 3, 1025, 8, 33, 0, 64], np.uint64)
    widths = np.array([classes[k % 10][0] for k in range(len(lengths))], np.uint8)
    preds = np.array([classes[k % 10][1] for k in range(len(lengths))], np.uint8)
    sub = layout._sub_lengths(lengths, widths)
    sizes = [int(n) + 5 if n else 0 for n in sub]  # a stream per sub-item with bytes
    sizes8, k = np.zeros(8 * len(lengths), np.int64), 0
    for i, w in enumerate(widths):
        sizes8[8 * i: 8 * i + int(w)] = sizes[k: k + int(w)]
        k += int(w)
    offsets8 = np.concatenate([[0], np.cumsum(sizes8)]).astype(np.uint64)
    offsets = tsp.compact_offsets(widths, offsets8)
    assert len(offsets) == int(widths.sum()) + 1 and [int(x) for x in np.diff(offsets.astype(np.int64))] == sizes
    payload = rs.randint(0, 256, int(offsets[-1])).astype(np.uint8)
    blob = layout.typed_items_header_bytes(rcx.CODER_ADAPTIVE, lengths, widths, preds, offsets) + payload.tobytes()
    c = layout.parse_typed_items(blob)
    assert np.array_equal(c["lengths"], lengths) and np.array_equal(c["widths"], widths) and np.array_equal(c["preds"], preds)
    assert np.array_equal(c["offsets"], offsets) and np.array_equal(c["payload"], payload) and c["crcs"] is None and c.get("stored") is None
    assert np.array_equal(c["sub_first"], np.concatenate([[0], np.cumsum(widths.astype(np.int64))]))
    assert list(tsp.compact_offsets(np.zeros(0, np.uint8), np.zeros(1, np.uint64))) == [0]
    bad = offsets8.copy()
    bad[8 * 1 + 3:] += np.uint64(2)  # a stream in a slot behind item 1's width (2)
    with pytest.raises(ValueError, match="behind an item's width"):
        tsp.compact_offsets(widths, bad)
    with pytest.raises(ValueError, match="eight slots"):
        tsp.compact_offsets(widths, offsets8[:-1])


# ---- the rules, sanitized ------------------------------------------------------------------------------------------------------
def write_batches(path, batches):
    """Per batch `n count max_bytes src_cap dst_cap status position`, then per entry `src_at dst_at len width pred class place kept`,
    the last three and the batch's status and position from plan_numpy."""
    code = {rcx.OK: 0, rcx.E_CAPACITY: 1, rcx.E_CORRUPT: 2}
    with open(path, "w") as f:
        f.write(f"{len(batches)}\n")
        for a, b, n, w, p, count, max_bytes, src_cap, dst_cap in batches:
            m = tsp.plan_numpy(a, b, n, w, p, count, max_bytes, src_cap, dst_cap)
            f.write(f"{len(n)} {count} {max_bytes} {src_cap} {dst_cap} {code[m['status']]} {-1 if m['position'] is None else m['position']}\n")
            for k in range(len(n)):
                f.write(f"{int(a[k])} {int(b[k])} {int(n[k])} {int(w[k])} {int(p[k])} {int(m['klass'][k])} {int(m['place'][k])} {int(m['kept'][k])}\n")


def test_rules_in_a_sanitized_program(tmp_path):
    """tests/sim/typed_split_picks_san.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: the 25 batches of the typed item
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
    exe, cases = str(tmp_path / "typed_split_picks_san"), str(tmp_path / "batches.txt")
    write_batches(cases, batches)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sim", "typed_split_picks_san.cpp")], check=True)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"typed_split_picks_san ok: {len(batches)} batches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
