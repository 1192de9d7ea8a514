"""The block statistics as far as they go without a GPU: the header against stats.EXPORTS and the built library, the
arithmetic of include/rcx_stats.h in its numpy form (stats.log2_q16, stats.cost_numpy), the rule of
pack_typed(predict="auto") on the typed buffers of DESIGN.md sections 11 to 13 -- with the CPU oracle: the rule takes what
codes smallest, and a cost is a little below what the adaptive coder makes of the same blocks -- and what is refused
before a GPU is needed."""
import os
import re

import numpy as np
import pytest

import planes_cases as pc
import predict_cases as pr
import stats_cases as sc
from cpprcoder_amd import container, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_stats.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, rcx
    build.build()
    names = declared_symbols()
    assert len(names) == 4 and set(names) == set(stats.EXPORTS), (names, stats.EXPORTS)
    for name in names:
        assert getattr(stats.lib(), name).argtypes is not None
    assert '#include "rcx.h"' in open(os.path.join(ROOT, "include", "rcx_stats.h")).read()
    # rcx.h, rcx_planes.h and rcx_predict.h are what they were
    assert len(rcx.EXPORTS) == 57 and len(planes.EXPORTS) == 4 and len(predict.EXPORTS) == 4 and rcx.lib().rcx_version() == 300
    assert not set(stats.EXPORTS) & (set(rcx.EXPORTS) | set(planes.EXPORTS) | set(predict.EXPORTS))
    assert all(h in build.HEADERS for h in ("rcx_stats.hpp", "rcx_stats_api.hpp")) and any(h.endswith("rcx_stats.h") for h in build.HEADERS)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------
PINS = ((1, 0), (2, 65536), (3, 103872), (256, 524288), (65536, 1048576), ((1 << 24) - 256, 1572862))


def test_log2_q16_pins_monotony_and_distance_to_the_logarithm():
    assert [int(v) for v in stats.log2_q16([x for x, _ in PINS])] == [want for _, want in PINS]
    assert int(stats.log2_q16(1 << 24)) == 24 << 16
    low = stats.log2_q16(np.arange(1, (1 << 18) + 1))
    assert bool((np.diff(low.astype(np.int64)) >= 0).all())
    rs = np.random.RandomState(16)
    x = np.concatenate([np.arange(1, 1 << 12), rs.randint(1, 1 << 24, 100_000), np.arange((1 << 24) - 5000, (1 << 24) + 1)]).astype(np.uint64)
    # never above log2, less than 2 units of 2^-16 below it (float64 has 52 bits for a figure below 2^21: exact enough)
    gap = np.log2(x.astype(np.float64)) * 65536.0 - stats.log2_q16(x).astype(np.float64)
    print("log2_q16 below log2 by", gap.min(), "..", gap.max())
    assert gap.min() >= 0 and gap.max() < 2
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(ValueError):
            stats.log2_q16(bad)


def test_cost_numpy_on_the_two_ends():
    one = np.zeros((3, 256), np.uint64)
    one[0, 0], one[1, 255], one[2, 17] = 1, 65536, (1 << 24) - 256
    assert [int(v) for v in stats.cost_numpy(one)] == [0, 0, 0]
    assert int(stats.cost_numpy(np.zeros(256, np.uint32))) == 0  # an empty item
    for each in (1, 16, 256, 65535):
        m = 256 * each
        assert int(stats.cost_numpy(np.full(256, each, np.uint32))) == m * 8 * 65536, each
    # two values, equally often: one bit a byte; and the restatement with bincount agrees with itself over blocks
    two = np.zeros(256, np.uint32)
    two[[0, 255]] = 2048
    assert int(stats.cost_numpy(two)) == 4096 * 65536
    x = np.random.RandomState(4).randint(0, 7, 3 * 100 + 31, dtype=np.uint8)
    h = sc.hist_blocks(x, 100)
    assert h.shape == (4, 256) and [int(v) for v in h.sum(axis=1)] == [100, 100, 100, 31]
    assert np.array_equal(h, sc.hist_items(x, np.array([0, 100, 200, 300, 331])))
    assert np.array_equal(stats.cost_numpy(h), [int(stats.cost_numpy(row)) for row in h])
    with pytest.raises(ValueError):
        stats.cost_numpy(np.zeros(255))


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_pick_predictor_margin_and_tie():
    pick = container.pick_predictor
    assert pick(6400, 6299, 6400) == "delta" and pick(6400, 6300, 6300) is None  # 64 * C_p < 63 * C_none, strictly
    assert pick(6400, 6400, 6299) == "zigzag" and pick(6400, 100, 100) == "delta" and pick(6400, 101, 100) == "zigzag"
    assert pick(0, 0, 0) is None and pick(1 << 60, (1 << 60) - (1 << 54) - 1, 1 << 60) == "delta"  # Python integers: no overflow


@pytest.fixture(scope="module")
def costs():
    """(buffer, block) -> (C_none, C_delta, C_zigzag) of its 1 MiB, computed once."""
    return {(name, block): sc.split_costs(*sc.typed_bytes(name), block) for name in sc.PICKS for block in (65536, 4096)}


def test_the_rule_picks_what_the_design_document_says(costs):
    """64 KiB blocks.  In bytes (nearest): sorted_keys 473449 / 234865 / 234887, csr_offsets 343960 / 98296 / 98296 (a tie:
    delta), random_walk 474907 / 348937 / 250640, signal 905177 / 575582 / 580397."""
    for name, want in sc.PICKS.items():
        c = costs[(name, 65536)]
        print(name, [sc.cost_bytes(v) for v in c], container.pick_predictor(*c))
        assert container.pick_predictor(*c) == want, (name, c)
    got = {name: tuple(sc.cost_bytes(v) for v in costs[(name, 65536)]) for name in pr.INTEGER_BUFFERS}
    assert got == {"sorted_keys": (473449, 234865, 234887), "csr_offsets": (343960, 98296, 98296), "random_walk": (474907, 348937, 250640),
                   "signal": (905177, 575582, 580397)}
    assert costs[("csr_offsets", 65536)][1] == costs[("csr_offsets", 65536)][2]
    # without the margin uniform bytes at 4 KiB blocks would take delta or zigzag for next to nothing
    c = costs[("uniform", 4096)]
    assert container.pick_predictor(*c) is None
    for name in ("indices", "bf16", "fp32"):
        assert container.pick_predictor(*costs[(name, 4096)]) is None


def test_the_rule_agrees_with_the_coder_and_a_cost_is_just_below_its_size(costs, oracle):
    """The adaptive coder at 64 KiB blocks through the CPU oracle.  The rule's pick is the predictor whose coded total is
    smallest, for all eight buffers (none for the four that no predictor helps).  Every cost, in bytes, is below the coded
    total and within 5.73 % of it -- the worst measured on these 24 texts plus one point; the issue's "3 %" does not hold on
    its own figures (98296 against 103173).  Measured, (total - cost) / total in percent, none / delta / zigzag:
        sorted_keys 0.82 1.84 1.87    csr_offsets 1.22 4.73 4.73    random_walk 0.84 1.25 1.74    signal 0.36 0.63 0.62
        indices 1.68 1.18 1.57        bf16 0.50 0.47 0.47           fp32 0.33 0.32 0.32           uniform 0.22 0.22 0.22
    The adaptive coder starts every block from a flat model and learns it: about the same few hundred bytes a block, which
    weigh most where the block codes to least."""
    for name, want in sc.PICKS.items():
        x, width = sc.typed_bytes(name)
        c = costs[(name, 65536)]
        totals = [pc.total_size(oracle, pr.split_numpy(x, width, 65536, pred), 65536, 0) for pred in (pr.NONE, pr.DELTA, pr.ZIGZAG)]
        gaps = [round(100.0 * (t - sc.cost_bytes(v)) / t, 2) for t, v in zip(totals, c)]
        print(name, totals, [sc.cost_bytes(v) for v in c], gaps)
        smallest = (None, "delta", "zigzag")[int(np.argmin(totals))]  # (argmin: the first of equals, delta before zigzag)
        assert container.pick_predictor(*c) == want == smallest, (name, totals, c)
        for t, v in zip(totals, c):
            assert v < t * 8 * stats.UNIT and (t * 8 * stats.UNIT - v) * 10000 <= 573 * t * 8 * stats.UNIT, (name, t, sc.cost_bytes(v))


# ---- refusals and the command line -----------------------------------------------------------------------------------------
def test_auto_on_nothing_needs_no_gpu_and_the_refused_stay_refused():
    for data in (np.zeros(0, np.int32), np.zeros(0, np.int64)):
        blob = container.pack_typed(data, predict="auto")
        assert blob == container.pack_typed(data) and blob[4] == 1 and container.parse_typed(blob)["pred"] == 0
        assert container.unpack_typed(blob) == b""
    checked = container.pack_typed(np.zeros(0, np.int32), predict="auto", checksum=True)
    assert checked == container.pack_typed(np.zeros(0, np.int32), checksum=True) and checked[4] == 1
    assert set(container.PREDICTORS) == {None, "delta", "zigzag"} and container.AUTO == "auto"
    ints = np.arange(64, dtype=np.int64)
    for predict in ("xor", "none", 1, 2, True, "DELTA", ["delta"], b"delta", "AUTO", "Auto", b"auto", ["auto"], ("auto",), 0, 3.0):
        with pytest.raises(container.ContainerError):
            container.pack_typed(ints, predict=predict)
    for data, width in ((b"abcdefgh", None), (b"abcdefgh", 3), (np.zeros(8, np.uint8), None)):
        with pytest.raises(container.ContainerError):
            container.pack_typed(data, width, predict="auto")


def test_command_line_takes_auto_only_with_planes():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    assert ap.parse_args(["c", "--planes", "8", "--predict", "auto", "in", "out"]).predict == "auto"
    assert ap.parse_args(["t", "--planes", "2", "--predict", "auto", "--crc", "f"]).predict == "auto"
    for argv in (["c", "--predict", "auto", "in", "out"], ["t", "--predict", "auto", "f"], ["c", "--blksort", "--predict", "auto", "in", "out"],
                 ["t", "--blksort", "--predict", "auto", "f"], ["d", "--predict", "auto", "in", "out"], ["c", "--planes", "4", "--predict", "AUTO", "in", "out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
