"""The adaptive encoder's division as its arithmetic wave does it (csrc/rcx_lane.hpp EncLane::arith_i, csrc/rcx_mc.hpp):

    t = mulhi(range + inc, mul) >> sh

with multiplier and increment from the quad decoder's table (csrc/rcx_ctx.hpp rcx_divtab_k: inc = 0 where the entry's addend
is 0, else 1) and the shift worked out once for a chunk of 16 symbols.  In integer arithmetic, no GPU: for the totals and
the ranges the coder can reach, the add does not wrap and the quotient is range // total.

A range is f * t with f <= total - 255 (the other 255 counts are at least 1) and t = R // total for the range R before, so
the largest one a total allows is (total - 255) * (0xFFFFFFFF // total); renormalised, it is shifted left by 8, 16 or 24.
"""
import numpy as np

U64 = np.uint64
TOP = 1 << 32


def div_entries(d):
    """rcx_make_div_entry (csrc/rcx_divtab.hpp) for an array of divisors -> (mul, inc, shift), inc as rcx_divtab_k stores it."""
    d = np.asarray(d, dtype=U64)
    s = np.floor(np.log2(d.astype(np.float64))).astype(U64)  # exact: d < 2^25
    assert np.all((U64(1) << s) <= d) and np.all(d < (U64(2) << s))
    pow2 = (d & (d - U64(1))) == 0
    big = U64(1) << (U64(32) + s)
    down = big // d
    rem = big - down * d
    up = (d - rem) <= (U64(1) << s)  # the rounded-up reciprocal fits 32 bits and is exact
    mul = np.where(pow2, U64(0xFFFFFFFF), np.where(up, down + U64(1), down))
    inc = np.where(pow2, U64(1), np.where(up, U64(0), U64(1)))
    assert np.all(mul < U64(TOP))
    return mul, inc, s


def chunk_shift(total):
    """The shift as the arithmetic wave takes it: from the first total of the chunk of 16 symbols, 31 - clz(256 + i0)."""
    first = ((np.asarray(total, dtype=U64) - U64(256)) & ~U64(15)) + U64(256)
    return np.floor(np.log2(first.astype(np.float64))).astype(U64)


def totals():
    rs = np.random.RandomState(20)
    every = np.arange(256, (1 << 17) + 1, dtype=np.int64)
    powers = np.array([(1 << k) + d for k in range(8, 25) for d in (-1, 0, 1) if (1 << k) + d >= 256], dtype=np.int64)
    sample = rs.randint((1 << 17) + 1, 1 << 24, size=100000).astype(np.int64)
    return np.unique(np.concatenate([every, powers, sample])).astype(U64)


def ranges_for(total):
    """(name, ranges, valid): the ranges to try for every total, and where each is one (fits 32 bits).  A draw is f * t with
    f <= total - 255 and t <= 0xFFFFFFFF // total; the draws that are shifted have a t small enough for the shift."""
    rs = np.random.RandomState(21)
    tmax = U64(0xFFFFFFFF) // total
    largest = (total - U64(255)) * tmax
    everywhere = np.ones(len(total), bool)

    def draw(limit):
        f = (rs.randint(0, 1 << 30, size=len(total)).astype(U64) % (total - U64(255))) + U64(1)
        room = np.minimum(tmax, U64(limit - 1) // f)  # f * t < limit
        t = (rs.randint(0, 1 << 30, size=len(total)).astype(U64) % np.maximum(room, U64(1))) + U64(1)
        return f * t

    out = [("initial", np.full(len(total), 0xFFFFFF00, dtype=U64), everywhere), ("largest", largest, everywhere),
           ("draw", draw(TOP), everywhere)]
    for k in (8, 16, 24):
        for name, r in (("largest", largest), ("draw", draw(TOP >> k))):
            shifted = r << U64(k)
            out.append((f"{name} << {k}", shifted, shifted < U64(TOP)))
    return out


def test_entries_are_the_tables():
    # the three kinds of entry, by hand: a power of two, a round-up and a round-down reciprocal
    mul, inc, s = div_entries([256, 257, 263, 1 << 24])
    assert [int(x) for x in s] == [8, 8, 8, 24]
    assert (int(mul[0]), int(inc[0])) == (0xFFFFFFFF, 1) and (int(mul[3]), int(inc[3])) == (0xFFFFFFFF, 1)
    for i, d in ((1, 257), (2, 263)):
        down = (1 << 40) // d
        want = (down + 1, 0) if d - ((1 << 40) - down * d) <= 256 else (down, 1)
        assert (int(mul[i]), int(inc[i])) == want


def test_a_chunk_has_one_shift():
    total = totals()
    _, _, s = div_entries(total)
    assert np.array_equal(chunk_shift(total), s)


def test_no_wrap_and_exact_quotient():
    total = totals()
    assert total[0] == 256 and total[-1] == (1 << 24) + 1 and len(total) > 230000
    mul, inc, _ = div_entries(total)
    sh = chunk_shift(total)
    seen = 0
    for name, r, valid in ranges_for(total):
        if not valid.any():  # (the largest range of a total has 24 bits or more: it fits shifted by 8 at total 256 alone)
            continue
        d, rr, m, i, s = total[valid], r[valid], mul[valid], inc[valid], sh[valid]
        n = rr + i
        wraps = n >= U64(TOP)
        assert not wraps.any(), f"{name}: range + inc wraps for total {int(d[wraps][0])}, range {int(rr[wraps][0]):#x}"
        got = ((n * m) >> U64(32)) >> s
        bad = got != rr // d
        assert not bad.any(), f"{name}: total {int(d[bad][0])}, range {int(rr[bad][0]):#x}: {int(got[bad][0])}"
        seen += int(valid.sum())
    assert seen > 4 * len(total)  # (a count above 2^16 or 2^8 leaves no range that fits shifted by 16 or 24)


def test_initial_range_meets_increment_one():
    # symbol 0: total 256, a power of two, so the increment is 1 and 0xFFFFFF00 + 1 is the add the first symbol makes
    mul, inc, s = div_entries([256])
    assert int(inc[0]) == 1 and ((0xFFFFFF01 * int(mul[0])) >> 32) >> int(s[0]) == 0xFFFFFF00 // 256
