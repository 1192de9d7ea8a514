"""The quad decoder's divisors (rcx_quad.hpp, RCX_QUAD_DIVQ_DW): multiplier and increment per symbol from global memory,
the shift per group of 16 symbols.

Round trips through the device entry points at the places that arrangement depends on: block lengths around the totals
that are powers of two (where the shift changes, and the entries whose addend is the multiplier), the symbol-by-symbol tail
(a ragged last block, an unaligned output), and every launch shape (1 .. 16 blocks per wave, one wave and two workgroups per
SIMD).  The encoder is held to the oracle elsewhere, so decode(encode(x)) == x is the decoder's bar here.
"""
import numpy as np
import pytest

from cpprcoder_amd import workloads
from gpu_support import ctx, round_trip_on_device  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def lengths_around_powers_of_two(top):
    """Symbol counts i where the total 256 + i is a power of two, and next to them (either side of a group of 16)."""
    out = []
    k = 9
    while (1 << k) - 256 <= top:
        edge = (1 << k) - 256
        out += [v for v in (edge - 17, edge - 16, edge - 1, edge, edge + 1, edge + 15, edge + 16, edge + 17) if 0 < v <= top]
        k += 1
    return out


@pytest.mark.parametrize("wl", ["uniform", "zipf"])
def test_single_blocks_across_shift_changes(ctx, wl):
    block = 1 << 18
    for i, n in enumerate(lengths_around_powers_of_two(block)):
        data = workloads.by_name(wl, n, 77 + i)
        back, st = round_trip_on_device(ctx, data, block)
        assert st == 0 and np.array_equal(back, data), f"{wl}, {n} bytes"


@pytest.mark.parametrize("block", [4096, 65536])
def test_wave_with_a_ragged_block_across_a_shift_change(ctx, block):
    # 16 blocks in one wave; the last one stops just past a power-of-two total, so the wave's fast loop ends there and
    # the rest of the other blocks is decoded symbol by symbol
    for last in ((1 << 11) - 256 + 3, (1 << 12) - 256 - 1, block - 1):
        n = 15 * block + last
        data = workloads.by_name("zipf", n, last)
        back, st = round_trip_on_device(ctx, data, block)
        assert st == 0 and np.array_equal(back, data), f"block {block}, last {last}"


@pytest.mark.parametrize("block", [4096, 16384])
def test_unaligned_output_runs_all_symbols_through_the_tail(ctx, block):
    n = 40 * block + 999
    data = workloads.by_name("uniform", n, block)
    back, st = round_trip_on_device(ctx, data, block, dst_offset=3)
    assert st == 0 and np.array_equal(back, data)


@pytest.mark.parametrize("nblocks", [1, 2, 3, 1000, 4096, 16384, 32768, 40000])
def test_every_launch_shape(ctx, nblocks):
    block = 4096
    n = nblocks * block - 100
    data = workloads.by_name("zipf" if nblocks % 2 else "uniform", n, nblocks)
    back, st = round_trip_on_device(ctx, data, block)
    assert st == 0 and np.array_equal(back, data), f"{nblocks} blocks"
