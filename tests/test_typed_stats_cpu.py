"""The candidate costs (include/rcx_typed_stats.h) and the containers that decide with them, where no GPU is needed: the header,
the exports and the library; what the pure check refuses; the numpy mirror on the header's example; the rule; the documents'
table; the crafted state dict decided from the mirror and coded by the CPU oracle; the refusals of the Python layer.

The host plan of csrc/rcx_typed_stats.hpp has no mapping function of its own -- it sorts the items by width and length, and the
kernel walks each item from its first byte with the index arithmetic of one item -- so there is no sanitized program here."""
import os
import re

import numpy as np
import pytest

import base_items_cases as bc
import stored_items_cases as sic
import typed_stats_cases as tsc
from cpprcoder_amd import base_items as bi, container, rcx, stats, typed_items, typed_stats as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = container.ContainerError

SOURCE = bytes.fromhex("05 01 00 01 42 00 AA 01 00 03 00 06 00 FF FF 02 00 AA")  # include/rcx_base_items.h's two items
BASE = bytes.fromhex("EE EE 00 01 02 01 42 00 55")
OFFS, BOFFS, WIDTHS = [0, 7, 18], [2, 1 << 40], [2, 2]


def L(x):
    return int(stats.log2_q16([x])[0])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_exports_and_library_agree():
    from cpprcoder_amd import base, build, planes, predict, stored, stored_items
    build.build()
    text = open(os.path.join(ROOT, "include", "rcx_typed_stats.h")).read()
    names = sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert len(names) == 3 and set(names) == set(ts.EXPORTS), (names, ts.EXPORTS)
    for name in names:
        assert getattr(ts.lib(), name).argtypes is not None
    assert '#include "rcx_base_items.h"' in text and '#include "rcx_stats.h"' in text
    for c, name in enumerate(("NONE", "DELTA", "ZIGZAG", "XOR", "SUB", "SUBZZ")):
        assert re.search(rf"#define RCX_CAND_{name} {c}\b", text) and getattr(ts, name) == c
    assert re.search(r"#define RCX_CANDS 6\b", text) and ts.CANDS == 6 and container.CANDIDATES == ts.NAMES
    assert [container.PREDICTORS[n] for n in ts.NAMES[:3]] == [0, 1, 2] and [container.BASE_OPS[n] + 3 for n in ts.NAMES[3:]] == [3, 4, 5]
    # rcx.h and the other headers are what they were, and no name is shared
    assert len(rcx.EXPORTS) == 57 and len(bi.EXPORTS) == 6 and len(stats.EXPORTS) == 4
    others = set(rcx.EXPORTS)
    for module in (planes, predict, stats, stored, stored_items, typed_items, base, bi):
        others |= set(module.EXPORTS)
    assert not set(ts.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_typed_stats.hpp", "rcx_typed_stats_api.hpp")) and any(h.endswith("rcx_typed_stats.h") for h in build.HEADERS)
    assert '#include "rcx_typed_stats_api.hpp"' in open(os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_api.hip")).read()


def test_check_refuses_each_case_and_accepts_its_neighbour():
    ok, bad = rcx.OK, rcx.E_ARG
    assert ts.check(OFFS, BOFFS, WIDTHS, [ts.ALL, ts.ALL_PREDS]) == ok
    assert ts.check(OFFS, BOFFS, WIDTHS, [0, 0]) == ok and ts.check([0], None, [], []) == ok
    # the shared tables: what rcx_base_items_check refuses
    assert ts.check([0, 7, 6], BOFFS, WIDTHS, [1, 1]) == bad and ts.check([0, 7, 7], BOFFS, WIDTHS, [1, 1]) == ok        # not ascending
    assert ts.check(OFFS, BOFFS, [2, 3], [1, 1]) == bad and ts.check(OFFS, BOFFS, [2, 4], [1, 1]) == ok                  # a width
    top = rcx.MAX_BLOCK
    assert ts.check([0, top + 1], None, [1], [1]) == bad and ts.check([0, top], None, [1], [1]) == ok                    # an item's length
    assert ts.check([0, 8 * top + 8], None, [8], [1]) == bad and ts.check([0, 8 * top + 7], None, [8], [1]) == bad and ts.check([0, 8 * top], None, [8], [1]) == ok
    # the masks
    assert ts.check(OFFS, BOFFS, WIDTHS, None) == bad
    assert ts.check(OFFS, BOFFS, WIDTHS, [0x40, 0]) == bad and ts.check(OFFS, BOFFS, WIDTHS, [0x20, 0]) == ok             # a bit at or above 6
    assert ts.check(OFFS, BOFFS, [1, 2], [2, 0]) == bad and ts.check(OFFS, BOFFS, [1, 2], [4, 0]) == bad                 # a predictor bit at width 1
    assert ts.check(OFFS, BOFFS, [1, 2], [ts.ALL_OPS, 2]) == ok
    assert ts.check(OFFS, None, WIDTHS, [8, 0]) == bad and ts.check(OFFS, None, WIDTHS, [ts.ALL_PREDS, 7]) == ok           # an op bit and no base offsets
    assert ts.check([0, 0, 11], None, WIDTHS, [8, 1]) == ok                                                             # ... on an item without bytes
    wrap = (1 << 64) - 8  # item 0 has 7 bytes
    assert ts.check(OFFS, [wrap + 1, 0], WIDTHS, [8, 0]) == bad and ts.check(OFFS, [wrap, 0], WIDTHS, [8, 0]) == ok       # a span that wraps
    assert ts.check(OFFS, [wrap + 1, 0], WIDTHS, [7, 0]) == ok                                                          # ... which nobody asked for


# ---- the mirror -------------------------------------------------------------------------------------------------------------------
def test_worked_example_pins_the_mirror():
    """The two items of include/rcx_base_items.h, as include/rcx_typed_stats.h writes them out."""
    got = ts.costs_numpy(SOURCE, BASE, OFFS, BOFFS, WIDTHS, [ts.ALL_OPS, ts.ALL_PREDS])
    none0 = 3 * L(3) + (4 * L(4) - 2 * L(2))        # 05 00 42 | 01 01 00 AA
    zz0 = 3 * L(3) + (4 * L(4) - 3 * L(3))          # 0A 03 00 | 00 00 00 AA, and xor's 05 02 00 | 00 00 00 AA
    sub0 = 3 * L(3) + (4 * L(4) - 2 * L(2))         # 05 FE 00 | 00 FF 00 AA
    delta1 = (5 * L(5) - 2 * L(2)) + (6 * L(6) - 4 * L(4))  # 01 02 03 F9 03 | 00 00 00 FF 00 AA
    assert (none0, zz0) == (311616 + 393216, 311616 + 212672)
    assert got[0].tolist() == [none0, 0, 0, zz0, sub0, zz0]
    assert got[1, 1] == delta1 and got[1, 3:].tolist() == [0, 0, 0] and got[1, 0] > 0 and got[1, 2] > 0
    # it is the composition, candidate by candidate
    for c, (preds, ops) in enumerate([(None, None), ([0, 1], None), ([0, 2], None), (None, [0, 0xFF]), (None, [1, 0xFF]), (None, [2, 0xFF])]):
        y = bi.split_numpy(SOURCE, BASE, OFFS, BOFFS, WIDTHS, preds, ops)
        so = typed_items.sub_offsets_numpy(OFFS, WIDTHS).astype(np.int64)
        cost = [int(stats.cost_numpy(np.bincount(y[so[k]: so[k + 1]], minlength=256))) for k in range(4)]
        for i in (0, 1):
            if [ts.ALL_OPS, ts.ALL_PREDS][i] >> c & 1:
                assert int(got[i, c]) == cost[2 * i] + cost[2 * i + 1], (i, c)
    with pytest.raises(ValueError):
        ts.costs_numpy(SOURCE, BASE, OFFS, BOFFS, [1, 2], [2, 0])
    assert ts.costs_numpy(b"", None, [0], None, [], []).shape == (0, 6)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
# the eight rows of DESIGN.md section 13: cost under none, delta, zigzag, and the pick
SECTION_13 = [(473_449, 234_865, 234_887, "delta"), (343_960, 98_296, 98_296, "delta"), (474_907, 348_937, 250_640, "zigzag"), (905_177, 575_582, 580_397, "delta"),
              (255_714, 360_152, 268_849, None), (697_594, 736_126, 733_340, None), (869_255, 892_075, 890_649, None), (1_048_199, 1_048_204, 1_048_200, None)]


def test_pick_candidate():
    rs = np.random.RandomState(5)
    for *t, pick in SECTION_13:
        assert container.pick_candidate(t + [0, 0, 0], ts.ALL_PREDS) == pick == container.pick_predictor(*t)
    triples = [(1000, 984, 984), (1000, 985, 984), (1000, 984, 983), (0, 0, 0), (64, 62, 63)] + [tuple(int(v) for v in rs.randint(0, 70, 3)) for _ in range(2000)] + [tuple(int(v) for v in rs.randint(900, 1100, 3)) for _ in range(2000)]
    for t in triples:  # on the predictors alone it is pick_predictor
        assert container.pick_candidate(list(t) + [0, 0, 0], ts.ALL_PREDS) == container.pick_predictor(*t), t
    # ties: delta, zigzag, subzz, sub, xor -- what needs no base first, subzz the default among the ops
    order = ["delta", "zigzag", "subzz", "sub", "xor"]
    number = {n: c for c, n in enumerate(ts.NAMES)}
    for k, first in enumerate(order):
        mask = 1 | sum(1 << number[n] for n in order[k:])
        assert container.pick_candidate([1000, 10, 10, 10, 10, 10], mask) == first
    assert container.pick_candidate([1000, 11, 11, 10, 11, 11]) == "xor"      # the cheapest wins before the order does
    assert container.pick_candidate([1000, 1, 1, 500, 400, 600], ts.ALL_OPS) == "sub"  # what was not asked for is not looked at
    # the margin of 1/64, on both sides of the border: 64 * C < 63 * C_none
    assert container.pick_candidate([6400, 9999, 9999, 6299, 9999, 9999]) == "xor" and container.pick_candidate([6400, 9999, 9999, 6300, 9999, 9999]) is None
    assert container.pick_candidate([64, 64, 64, 63, 64, 62]) == "subzz" and container.pick_candidate([64, 64, 64, 63, 63, 63]) is None
    assert container.pick_candidate([0] * 6) is None and container.pick_candidate([0, 5, 5, 5, 5, 5]) is None
    with pytest.raises(E):
        container.pick_candidate([1] * 6, ts.OP_BITS)
    # pack_delta's rule among the three ops: the cheapest, ties subzz, sub, xor, no margin
    assert container.pick_op(5, 5, 5) == "subzz" and container.pick_op(5, 5, 6) == "sub" and container.pick_op(5, 6, 6) == "xor"
    assert container.pick_op(7, 6, 5) == "subzz" and container.pick_op(0, 0, 0) == "subzz"


# ---- the documents' table ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """name -> (the row's tables, the costs per item from the mirror)"""
    out = {}
    for name, data, base, width, pick, tie in tsc.table_rows():
        x, offs, widths, masks = tsc.row_tables(data, width)
        ref = np.ascontiguousarray(base).reshape(-1).view(np.uint8)
        out[name] = (x, ref, offs, widths, masks, pick, tie, ts.costs_numpy(x, ref, offs, offs[:-1], widths, masks))
    return out


def test_the_table_of_the_documents_gives_its_picks(table):
    assert len(table) == 9
    for name, (x, ref, offs, widths, masks, pick, tie, costs) in table.items():
        sums = [int(v) for v in costs.sum(axis=0, dtype=np.uint64)]
        print(name, [s >> 19 for s in sums])
        assert container.pick_candidate(sums, int(masks[0])) == pick, name
        if tie:
            assert sums[ts.SUB] == sums[ts.SUBZZ], name
        # the decision per item, from the same table: every item of these rows goes the way its tensor goes
        ops, preds = container.choose_delta_items_from_costs(costs, [True] * len(widths), widths, "auto", "auto" if int(widths[0]) > 1 else None)
        assert set(ops) | set(preds) == {pick, None}, name
    first = table["bf16 moved"][-1].sum(axis=0, dtype=np.uint64) >> np.uint64(19)
    assert first.tolist() == [697_574, 736_333, 733_515, 271_080, 295_962, 236_224]  # the row the issue quotes


# rows in which another asked candidate lies within 1/64 of the pick's cost: the order-0 estimate cannot rank those, and the
# assertion below leaves them out by the rule's own margin
WITHIN_MARGIN = {"uint8 unrelated", "sorted int64"}  # all four of uint8 unrelated; delta and zigzag of sorted int64


def test_the_pick_codes_smallest_with_the_oracle(oracle, table):
    """For each row whose pick is not a tie, the pick's total as the CPU oracle codes it is the smallest of the asked
    candidates.  Left out: the ties (fp32 identical, uint64 counters, zeros) and the rows of WITHIN_MARGIN."""
    checked = 0
    for name, (x, ref, offs, widths, masks, pick, tie, costs) in table.items():
        sums = [int(v) for v in costs.sum(axis=0, dtype=np.uint64)]
        c_pick = sums[ts.NAMES.index(pick)]
        near = [c for c in range(6) if int(masks[0]) >> c & 1 and ts.NAMES[c] != pick and 64 * min(sums[c], c_pick) >= 63 * max(sums[c], c_pick)]
        assert (name in WITHIN_MARGIN) == bool(near and not tie and name != "zeros"), (name, near)
        if tie or name == "zeros" or name in WITHIN_MARGIN:
            continue
        so = typed_items.sub_offsets_numpy(offs, widths).astype(np.int64)
        coded = {}
        for c in range(6):
            if not int(masks[0]) >> c & 1:
                continue
            preds = np.full(len(widths), c, np.uint8) if c in (1, 2) else None
            ops = np.full(len(widths), c - 3, np.uint8) if c >= 3 else None
            y = bi.split_numpy(x, ref, offs, offs[:-1], widths, preds, ops)
            coded[ts.NAMES[c]] = len(sic.oracle_item_streams(oracle, [y[so[k]: so[k + 1]] for k in range(len(so) - 1)], 0)[0])
        print(name, coded)
        assert min(coded, key=lambda k: coded[k]) == pick, (name, coded)
        checked += 1
    assert checked == 4  # bf16 moved, bf16 unrelated, fp32 moved, uint8 flipped


# ---- the crafted state dict -----------------------------------------------------------------------------------------------------
def oracle_container(oracle, t):
    """test_base_items_cpu.oracle_container for the delta container: the RCXK the device path writes, with the mirror and the
    CPU oracle -> (blob, payload bytes per item)"""
    import zlib
    offs = tsc.offsets_of(t["lengths"])
    y = bi.split_numpy(t["x"], t["ref"], offs, t["base_offsets"], t["widths"], t["preds"], t["ops"])
    soffs = typed_items.sub_offsets_numpy(offs, t["widths"]).astype(np.int64)
    payload, offsets = sic.oracle_item_streams(oracle, [y[soffs[k]: soffs[k + 1]] for k in range(len(soffs) - 1)], 0)
    inner = container.typed_items_header_bytes(0, t["lengths"], t["widths"], t["preds"], offsets, None, b"") + payload.tobytes()
    per_sub = np.diff(offsets.astype(np.int64))
    first = np.concatenate([[0], np.cumsum(t["widths"].astype(np.int64))])
    per_item = np.array([per_sub[first[i]: first[i + 1]].sum() for i in range(len(t["widths"]))])
    crcs = [zlib.crc32(t["ref"][int(b): int(b) + int(n)].tobytes()) if op != bc.NO_BASE else 0 for b, n, op in zip(t["base_offsets"], t["lengths"], t["ops"])]
    return container.delta_items_header_bytes(t["ops"], crcs) + inner, per_item


def decide(named, base):
    """choose_tensors_delta(op="auto", predict="auto") from the mirror's table -> (op, predict, the costs per item, the tables)"""
    m = container.tensor_delta_masks(named, base, 65536, "auto", "auto")
    t = bc.tensor_items(named, base, 65536)  # (x, ref and base_offsets: every tensor the base holds is measured against it)
    assert t["lengths"].tolist() == m["lengths"].tolist() and t["widths"].tolist() == m["widths"].tolist()
    assert ((m["masks"] & ts.OP_BITS) != 0).tolist() == (t["ops"] != bc.NO_BASE).tolist()
    costs = ts.costs_numpy(t["x"], t["ref"], tsc.offsets_of(t["lengths"]), t["base_offsets"], t["widths"], m["masks"])
    op, predict = container.choose_tensors_delta_from_costs(costs, named, base, 65536, "auto", "auto")
    return op, predict, costs, m


def test_the_crafted_state_dict_decides_for_itself(oracle):
    named, before, _ = bc.state_dicts()
    op, predict, costs, m = decide(named, before)
    assert m["masks"].tolist() == [ts.ALL] * 8 + [ts.ALL_PREDS] * 2 and m["first"]["embed.frozen"] == (7, 1)
    assert op == {"layer0.weight": "subzz", "layer1.weight": "subzz", "embed.frozen": "subzz", "head.new": None, "index.sorted": None}
    assert predict == {"layer0.weight": None, "layer1.weight": None, "embed.frozen": None, "head.new": None, "index.sorted": "delta"}
    t = bc.tensor_items(named, {k: v for k, v in before.items() if op[k]}, 65536, bi.SUBZZ, predict)
    blob, _ = oracle_container(oracle, t)
    print(len(blob))
    assert len(blob) <= 432_890  # what the named choices of tests/test_base_items_cpu.py give: here the same choices, measured


def test_a_tensor_against_an_unrelated_base_decides_none(oracle):
    """layer0.weight (moved by randn * 1e-4) against a base replaced by unrelated values: no base, and its payload is then the
    RCXJ payload of that tensor."""
    named, before, _ = bc.state_dicts()
    name = "layer0.weight"
    other = np.random.default_rng(3).integers(0, 1 << 16, named[name].shape).astype(np.uint16)
    op, predict, costs, m = decide({name: named[name]}, {name: other})
    assert op == {name: None} and predict == {name: None}
    sums = costs.sum(axis=0, dtype=np.uint64)
    assert all(64 * int(sums[c]) >= 63 * int(sums[0]) for c in range(1, 6))
    decided = bc.tensor_items({name: named[name]}, {}, 65536)
    assert decided["ops"].tolist() == [bc.NO_BASE] * 4 and len(decided["ref"]) == 0
    blob, per_item = oracle_container(oracle, decided)
    plain = bc.tensor_items({name: named[name]}, {}, 65536)
    so = typed_items.sub_offsets_numpy(tsc.offsets_of(plain["lengths"]), plain["widths"]).astype(np.int64)
    y = typed_items.split_numpy(plain["x"], tsc.offsets_of(plain["lengths"]), plain["widths"], None)
    payload, _ = sic.oracle_item_streams(oracle, [y[so[k]: so[k + 1]] for k in range(len(so) - 1)], 0)
    c = container.parse_delta_items(blob)
    assert c["ops"].tolist() == [bc.NO_BASE] * 4 and bytes(c["inner"]["payload"]) == payload.tobytes()
    # against its own base the same tensor takes subzz
    assert decide({name: named[name]}, {name: before[name]})[0] == {name: "subzz"}


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_the_decision_from_a_table():
    costs = np.array([[100, 10, 10, 10, 10, 10], [100, 99, 99, 50, 40, 60], [100, 10, 10, 99, 99, 99], [100, 99, 99, 99, 99, 99], [7, 7, 7, 7, 7, 7]], np.uint64)
    has, widths = [True, True, False, True, True], [2, 2, 4, 8, 1]
    assert container.delta_item_masks(has, widths, "auto", "auto").tolist() == [ts.ALL, ts.ALL, ts.ALL_PREDS, ts.ALL, ts.ALL_OPS]
    assert container.delta_item_masks(has, widths, "auto", None).tolist() == [ts.ALL_OPS, ts.ALL_OPS, 0, ts.ALL_OPS, ts.ALL_OPS]
    assert container.delta_item_masks(has, widths, ["auto", "xor", None, None, "auto"], [None, None, "auto", "delta", None]).tolist() == [ts.ALL_OPS, 0, 7, 0, ts.ALL_OPS]
    ops, preds = container.choose_delta_items_from_costs(costs, has, widths, "auto", "auto")
    assert ops == [None, "sub", None, None, None] and preds == ["delta", None, "delta", None, None]
    ops, preds = container.choose_delta_items_from_costs(costs, has, widths, "auto", None)  # the predictors are not looked at
    assert ops == ["subzz", "sub", None, None, None] and preds == [None] * 5
    ops, preds = container.choose_delta_items_from_costs(costs, has, widths, ["auto", "xor", None, None, "auto"], [None, None, "zigzag", "delta", None])
    assert ops == ["subzz", "xor", None, None, None] and preds == [None, None, "zigzag", "delta", None]
    ops, preds = container.choose_delta_items_from_costs(costs, has, widths, "auto", "zigzag")  # a named predictor is for the items without a base
    assert ops == ["subzz", "sub", None, None, None] and preds == [None, None, "zigzag", None, None]


def test_what_the_python_layer_refuses_before_it_needs_a_gpu():
    x, b = np.arange(8, dtype=np.uint16), np.arange(8, dtype=np.uint16)
    for bad in (lambda: container.pack_delta_items([x, x], [b, None], ops=["auto", "auto"]),                     # "auto" and no base
                lambda: container.choose_delta_items([x, x], [b, None], ops=["sub", "auto"]),
                lambda: container.pack_delta_items([x, x], [b, None], ops=["auto", None], predict=["delta", None]),  # a named predictor on an auto item
                lambda: container.choose_delta_items([x], [b], ops=["auto"], predict=["zigzag"]),
                lambda: container.pack_delta_items([x, x], [b, b], ops=["auto", "minus"]), lambda: container.pack_delta_items([x, x], [b, b], ops=["auto", 2]),
                lambda: container.pack_delta_items([x], [b], ops="auto", predict="plus"), lambda: container.pack_delta_items([x], [b], ops=["auto"], predict=["Auto"]),
                lambda: container.pack_delta_items([x, x], [b, b], ops=["auto"]), lambda: container.pack_delta_items([x], [b[:7]], ops="auto"),
                lambda: container.choose_delta_items_from_costs(np.zeros((1, 6)), [False], [2], ops=["auto"]),
                lambda: container.pack_tensors_delta({"a": x}, {}, op={"a": "auto"}),                              # "auto" by name, and the base lacks it
                lambda: container.pack_tensors_delta({"a": x}, {"a": b}, op={"a": "automatic"}), lambda: container.pack_tensors_delta({"a": x}, {"a": b}, op="auto", predict="plus"),
                lambda: container.pack_delta(x, b, op="Auto"), lambda: container.pack_delta(x, b[:7], op="auto")):
        with pytest.raises(E):
            bad()
    # nothing to measure: no GPU, the rule on costs of 0 says none, and the container is the one of the named choices
    empty = [b"", x[:0]], [b"", b[:0]]
    assert container.choose_delta_items(*empty, widths=[1, 2], ops="auto", predict="auto") == ([None, None], [None, None])
    assert container.pack_delta_items(*empty, widths=[1, 2], ops=["auto", "auto"]) == container.pack_delta_items(*empty, widths=[1, 2], ops=[None, None])
    # pack_delta_items measures per entry of the list; the one name "auto" for all items is an op name it never had, refused as before
    with pytest.raises(E):
        container.pack_delta_items([x], [b], ops="auto")
    assert container.choose_delta_items_from_costs(np.zeros((1, 6)), [True], [2], ops="auto") == ([None], [None])
    e = {"e": np.zeros((0, 3), np.float32)}
    assert container.pack_tensors_delta(e, e, op="auto", predict="auto") == container.pack_tensors_delta(e, e, op={"e": None})
    assert container.choose_tensors_delta(e, e) == ({"e": None}, {"e": None})
    assert container.pack_delta(b"", b"", 1, op="auto") == container.pack_delta(b"", b"", 1, op="subzz")


def test_base_op_auto_on_the_command_line():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    assert ap.parse_args(["c", "--base", "old.bin", "--base-op", "auto", "in", "out"]).base_op == "auto"
    assert ap.parse_args(["t", "--planes", "2", "--base", "old.bin", "--base-op", "auto", "f"]).base_op == "auto"
    for bad in (["c", "--base-op", "auto", "in", "out"], ["t", "--base-op", "auto", "f"], ["c", "--base", "old.bin", "--base-op", "Auto", "in", "out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
