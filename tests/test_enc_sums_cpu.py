"""The model waves' sums of a group of four counts (csrc/rcx_lane.hpp: rcx_pre4, rcx_pre4_sel4, rcx_sel4), as compiled for
the host (tests/sim/enc_sums_sim.cpp), against their plain definitions:

    rcx_pre4(g, p)  = g[0] + ... + g[p - 1]          the sum of the first p
    rcx_sel4(g, p)  = g[p]                           element p

The kernels form them as chains of 24-bit multiply-adds with the 0/1 factors (p > 0), (p > 1), (p > 2) -- the first p as
x m1 + y m2 + z m3, the first p + 1 as x + y m1 + z m2 + w m3, the count as their difference -- which is the same u32 value
as long as every count is below 2^24 (the multiply reads 24 bits of each factor).  Counts at and around 2^16 and up to
2^24 - 1, every p, and seeded random groups.  No GPU.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_SRC = os.path.join(ROOT, "tests", "sim", "enc_sums_sim.cpp")
SIM_SO = os.path.join(ROOT, "tests", "sim", "libencsumssim.so")

EDGES = (0, 1, 2, 65535, 65536, 65537, (1 << 24) - 257, (1 << 24) - 1)


@pytest.fixture(scope="module")
def sim():
    deps = [SIM_SRC, os.path.join(ROOT, "cpprcoder_amd", "csrc", "rcx_lane.hpp")]
    if not os.path.exists(SIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SIM_SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SIM_SO, SIM_SRC], check=True)
    L = C.CDLL(SIM_SO)
    L.sim_group_sums.restype = None
    L.sim_group_sums.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
    return L


def run(sim, groups):
    groups = np.ascontiguousarray(groups, dtype=np.uint32)
    out = [np.zeros((len(groups), 4), np.uint32) for _ in range(4)]
    sim.sim_group_sums(groups.ctypes.data, len(groups), *[o.ctypes.data for o in out])
    return out


def expected(groups):
    """(sums, counts), both n x 4, column p: the sum of the first p (mod 2^32, as u32 arithmetic has it) and element p."""
    g = np.asarray(groups, dtype=np.uint64)
    before = np.concatenate([np.zeros((len(g), 1), np.uint64), np.cumsum(g, axis=1)[:, :3]], axis=1)
    return (before & np.uint64(0xFFFFFFFF)).astype(np.uint32), g.astype(np.uint32)


def check(sim, groups):
    sums, counts, both_sums, both_counts = run(sim, groups)
    want_sums, want_counts = expected(groups)
    for name, got, want in (("rcx_pre4", sums, want_sums), ("rcx_sel4", counts, want_counts),
                            ("rcx_pre4_sel4 sum", both_sums, want_sums), ("rcx_pre4_sel4 count", both_counts, want_counts)):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name}: group {list(groups[bad[0][0]])}, p = {bad[0][1]}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def test_every_group_of_the_edge_counts(sim):
    groups = np.array(list(itertools.product(EDGES, repeat=4)), dtype=np.uint32)
    assert len(groups) == len(EDGES) ** 4
    check(sim, groups)


def test_random_groups_below_2_to_24(sim):
    rs = np.random.RandomState(21)
    groups = rs.randint(0, 1 << 24, size=(100000, 4)).astype(np.uint32)
    # a share of them small, as a block's counts are, and at every magnitude in between
    groups[:30000] >>= rs.randint(0, 24, size=(30000, 4)).astype(np.uint32)
    check(sim, groups)


def test_by_hand(sim):
    sums, counts, both_sums, both_counts = run(sim, [[5, 7, 11, 13]])
    assert sums.tolist() == both_sums.tolist() == [[0, 5, 12, 23]]
    assert counts.tolist() == both_counts.tolist() == [[5, 7, 11, 13]]
