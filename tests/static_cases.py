"""Inputs that put the static range coder (csrc/rcx_static.hpp) on its large totals and on the 16-bit squeeze of count()
(cpprcoder.h:543-571), with the models that say what each input is for.  Everything is seeded; every premise stated
here is asserted on the CPU against the oracle by tests/test_static_cases_cpu.py.

Large totals.  A decoder's total comes from the stream's header, not from the number of symbols, so streams made by
oracle.static_encode_table (static_encode with the caller's table) reach totals near 2^24 with short blocks:
tables(), crafted_blocks().  parent_estimate() restates the target low / t of the one-lane decoder as it was computed
before rcx_static_target (csrc/rcx_lane.hpp): one f32 estimate and a step of +-1, exact only for quotients below 2^21.

What that arithmetic gets wrong, and where a stream can meet it.  With the exactly rounded reciprocal, and with one
that is 1 ulp larger, every wrong target is floor(low / t) + 1.  That names another symbol only if low lies in the
topmost t of its symbol's interval [cum[c] t, cum[c + 1] t), and then the next symbol's low is within t of the top of
its range f t -- where no encoder puts a code unless the part of the range that the division leaves unused,
(f t 256) mod total, is smaller than that.  top_slivers() lists the (t, c) where it is: none at all for the near-flat
and the random table with the exactly rounded reciprocal, 22 for the near-flat tables at +1 ulp, thousands for the flat
and the half-zero table (f 256 is a multiple of their totals).  With a reciprocal 1 ulp smaller the wrong targets are
floor(low / t) - 1, the bottom of an interval, which every stream reaches: 14 of the 64 near-flat blocks are decoded
wrong then.  So whether the arithmetic fails on a valid stream depends on v_rcp_f32's actual rounding, which nobody has
measured, while a damaged stream, whose low lies anywhere, meets it with any reciprocal.  aimed_streams() are such
streams: valid ones whose first low is moved onto a target that parent_estimate gets wrong.

Squeeze.  squeeze_ladder() has blocks of 65536 + 1024 bytes whose dominant byte's 65536th occurrence -- the symbol in
front of which count() halves every count -- falls on each position of the first 16-byte piece that the encoders check,
in a later piece, on the block's first possible and its last symbol, blocks that stop just short of a squeeze, and three
that bracket the three-wave encoder's `calm` decision.  squeeze_points() is count() in Python.

natural_block() and natural_stream() are the two inputs whose own histogram has a total near 2^24.
"""
import functools

import numpy as np

import oracle_lib

NBLOCKS, BLOCK = 64, 262144   # crafted: one wave of the one-lane kernel per table
LADDER_BLOCK = 65536 + 1024   # a multiple of 16
EASY16 = 65520                # the symbols the three-wave encoder counts before it decides `calm` (65535 & ~15)
DOMINANT = 0x41

NEAR_FLAT = (65535 - (37 * np.arange(256) % 1024)).astype(np.uint32)


# ---- tables ------------------------------------------------------------------------------------------------------------
def tables():
    """name -> 256 counts.  The near-flat table at full, half and quarter scale (totals 16 647 552, 8 323 712,
    4 161 792); the flat table, whose t = range / total is a power of two every time, so that any reciprocal is exact (the
    degenerate case); counts drawn at random in [1, 65535]; and 128 counts of 0 among counts of 65535, whose equal
    cumulative counts meet the `<=` of find() (cpprcoder.h:521-535).

    The random counts are the larger of two uniform draws (mean 2/3 of 65535, total 11.3 M): the sum of 256 single
    uniform draws is 8.4 M +- 0.3 M, about 2^23, where the estimate that parent_estimate restates is still exact with an
    exactly rounded reciprocal, so such a table could not show what it is here to show."""
    rs = np.random.RandomState(20)
    zeros = np.full(256, 65535, np.uint32)
    zeros[rs.permutation(256)[:128]] = 0
    return {
        "near-flat": NEAR_FLAT,
        "near-flat/2": NEAR_FLAT >> 1,
        "near-flat/4": NEAR_FLAT >> 2,
        "flat": np.full(256, 65535, np.uint32),
        "random": np.maximum(rs.randint(1, 65536, 256), rs.randint(1, 65536, 256)).astype(np.uint32),
        "half-zero": zeros,
    }


LARGE = ("near-flat", "random", "half-zero", "flat")  # totals past 2^23


def draw(counts, n, rs):
    """n symbols from the distribution of the table."""
    cum = np.cumsum(counts.astype(np.int64))
    return np.searchsorted(cum, rs.randint(0, int(cum[-1]), n), side="right").astype(np.uint8)


def crafted_blocks(name, nblocks=NBLOCKS, n=BLOCK, trace=False):
    """-> [(data, stream)] or, with trace, an iterator of (data, stream, low, range): nblocks blocks of n symbols drawn
    from table `name`, each encoded by the oracle with that table; low / range = the decoder's state in front of every
    symbol.  (Without the traces the list is kept: 32 MiB a table.)"""
    if trace:
        return _crafted(name, nblocks, n, True)
    return _kept(name, nblocks, n)


@functools.lru_cache(maxsize=None)
def _kept(name, nblocks, n):
    return list(_crafted(name, nblocks, n, False))


def _crafted(name, nblocks, n, trace):
    counts = tables()[name]
    rs = np.random.RandomState(1000 + sorted(tables()).index(name))
    chk = oracle_lib.oracle()
    for _ in range(nblocks):
        data = draw(counts, n, rs)
        got = chk.static_encode_table(counts, data, trace=trace)
        yield (data, *got) if trace else (data, got)


# ---- the target as it was computed ---------------------------------------------------------------------------------------
def parent_estimate(low, t, ulp=0):
    """The one-lane static decoder's target low / t as computed before rcx_static_target: q = (u32)((float)low * rcp((float)t)),
    then one step of +-1 -- in numpy float32 (IEEE, as v_cvt_f32_u32 and v_mul_f32 are).  ulp: the exactly rounded
    reciprocal moved by that many ulp (+1, -1), the room v_rcp_f32's stated accuracy leaves.

    Over the traces of the crafted blocks (64 blocks x 262144 symbols a table) it differs from low // t in
        near-flat     353 951 targets at ulp = 0,  5 110 405 at +1,  664 861 at -1
        random         40 446                      1 587 749          34 947
        near-flat/2         0                        458 191           9 135
        half-zero           0                      1 048 047               0
        flat                0                      6 808 277               0
        near-flat/4         0                              0               0
    (tests/test_lane_sim.py counts them again), and names a wrong symbol in 14 near-flat and 3 random blocks at -1 ulp,
    in 53 flat and 16 half-zero blocks at +1 ulp, and in none otherwise: see the module's text."""
    low = np.asarray(low, np.uint32)
    t = np.asarray(t, np.uint32)
    r = (np.float32(1) / t.astype(np.float32)).astype(np.float32)
    if ulp:
        r = np.nextafter(r, np.float32(2 if ulp > 0 else 0)).astype(np.float32)
    q = (low.astype(np.float32) * r).astype(np.float32).astype(np.int64)
    prod = q * t.astype(np.int64)
    low64 = low.astype(np.int64)
    q = np.where(prod > low64, q - 1, np.where(low64 - prod >= t, q + 1, q))
    return q.astype(np.uint32)


def symbols_of(counts, targets):
    """find() (cpprcoder.h:521-535): how many of cum[1..255] are <= target."""
    cum = np.cumsum(counts.astype(np.int64))
    return np.minimum(np.searchsorted(cum[:255], np.asarray(targets).astype(np.int64), side="right"), 255)


def wrong_symbols(counts, low, rng, ulp=0):
    """One traced block -> (the symbols at which parent_estimate names another symbol than low // t does, how many targets
    it gets wrong)."""
    total = int(counts.astype(np.int64).sum())
    t = rng // np.uint32(total)
    want = low // t
    got = parent_estimate(low, t, ulp)
    off = np.nonzero(got != want)[0]
    return off[symbols_of(counts, got[off]) != symbols_of(counts, want[off])], len(off)


def wrong_blocks(name, ulps=(0,)):
    """{ulp: (the crafted blocks of table `name` in which parent_estimate decodes a wrong symbol, the targets it gets wrong
    in all of them)}, from the oracle's traces."""
    counts = tables()[name]
    out = {u: ([], 0) for u in ulps}
    for b, (_, _, low, rng) in enumerate(crafted_blocks(name, trace=True)):
        for u in ulps:
            symbols, targets = wrong_symbols(counts, low, rng, u)
            out[u] = (out[u][0] + ([b] if len(symbols) else []), out[u][1] + targets)
    return out


# table -> (ulp, the first crafted blocks, eight at the most, in which parent_estimate with that reciprocal names a wrong
# symbol): wrong_blocks() in short, held to it by tests/test_static_cases_cpu.py, for the tests that only want some such blocks
MARKED = {"near-flat": (-1, [6, 7, 13, 15, 17, 26, 31, 32]), "random": (-1, [47, 50, 52]),
          "flat": (1, [0, 1, 2, 3, 4, 5, 6, 7]), "half-zero": (1, [2, 9, 13, 18, 23, 31, 36, 37])}


def top_slivers(name, ulp):
    """The (t, c) at which a VALID stream can make parent_estimate name a wrong symbol by a target one too large: some low
    in the topmost t of symbol c's interval gets a wrong target, and the low that this leaves for the next symbol (shifted
    as the renormalisation shifts it) is below total * t', the part of the next range that an encoder uses."""
    counts = tables()[name].astype(np.int64)
    total = int(counts.sum())
    cum = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for t in range(1, 0xFFFFFFFF // total + 1):
        for c in np.nonzero(counts)[0]:
            lows = (int(cum[c + 1]) - 1) * t + np.arange(t, dtype=np.int64)
            wrong = np.nonzero(parent_estimate(lows, np.full(t, t), ulp) != lows // t)[0]
            if len(wrong) == 0:
                continue
            left, rng = int(lows[wrong[0]]) - int(cum[c]) * t, int(counts[c]) * t
            while rng < 1 << 24:
                rng, left = rng << 8, left << 8
            if left < total * (rng // total):
                out.append((t, int(c)))
    return out


def _wrong_lows(counts, t, ulp):
    """One low per symbol edge (the topmost and the lowest t of each interval) whose target parent_estimate gets wrong so that
    it names the neighbouring symbol."""
    cum = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    out = []
    for c in np.nonzero(counts)[0]:
        for q in (int(cum[c + 1]) - 1, int(cum[c])):
            lows = q * t + np.arange(t, dtype=np.int64)
            wrong = lows[symbols_of(counts, parent_estimate(lows, np.full(t, t), ulp)) != c]
            out.extend(int(x) for x in wrong[:1])
    return out


def aimed_streams(name, ulp, count=16, n=4096):
    """-> [stream, padded with 3 n seeded bytes] of n symbols each: valid streams of table `name` whose first bytes are
    replaced so that the low in front of the first or the second symbol is one whose target parent_estimate gets wrong with
    the reciprocal moved by `ulp`, at the top (target one too large) or the bottom (one too small) of a symbol's interval,
    so that it names the neighbour.  No encoder makes such a stream; the reference decodes it like any other (what follows
    is arbitrary but determined, and the padding lets it run to the end).  [] where neither symbol's t has such a low."""
    counts = tables()[name]
    c64 = counts.astype(np.int64)
    total = int(c64.sum())
    cum = np.concatenate([[0], np.cumsum(c64)])
    t0 = 0xFFFFFFFF // total
    aims = [(low, None) for low in _wrong_lows(counts, t0, ulp)]
    by_t = {}
    for c1 in np.nonzero(c64)[0]:  # the second symbol: behind c1 the range is f t0, shifted once where that is below 2^24
        if len(aims) >= 8 * count:
            break
        rng, shift = int(c64[c1]) * t0, 0
        while rng < 1 << 24:
            rng, shift = rng << 8, shift + 8
        t1 = rng // total
        if t1 not in by_t:
            by_t[t1] = _wrong_lows(counts, t1, ulp)
        for low1 in by_t[t1]:
            if shift <= 8 and low1 < rng:
                aims.append((int(cum[c1]) * t0 + (low1 >> shift), (low1 & 255) if shift else None))
    rs = np.random.RandomState(4000 + 10 * sorted(tables()).index(name) + ulp)
    chk = oracle_lib.oracle()
    out = []
    for i in rs.permutation(len(aims))[:count]:
        low, after = aims[i]
        s = chk.static_encode_table(counts, draw(counts, n, rs))
        s[517:521] = [low >> 24, (low >> 16) & 255, (low >> 8) & 255, low & 255]
        if after is not None:
            s[521] = after
        out.append(np.concatenate([s, rs.randint(0, 256, 3 * n).astype(np.uint8)]))
    return out


def parent_decodes(counts, stream, symbols, ulp):
    """The first `symbols` symbols of a stream as the one-lane decoder named them with parent_estimate (cpprcoder.h:500-517,
    in Python)."""
    c64 = counts.astype(np.int64)
    total = int(c64.sum())
    cum = np.concatenate([[0], np.cumsum(c64)])
    low, rng, at, out = int.from_bytes(bytes(stream[517:521]), "big"), 0xFFFFFFFF, 521, []
    for _ in range(symbols):
        t = rng // total
        target = int(parent_estimate([low], [t], ulp)[0]) if low < total * t else 0xFFFFFFFF
        c = int(symbols_of(counts, [target])[0])
        out.append(c)
        low, rng = (low - int(cum[c]) * t) & 0xFFFFFFFF, int(c64[c]) * t
        if rng == 0:  # a symbol of count 0: the reference runs dry here
            break
        while rng < 1 << 24:
            low, rng, at = ((low << 8) | int(stream[at])) & 0xFFFFFFFF, rng << 8, at + 1
    return out


# ---- count() and its squeeze ---------------------------------------------------------------------------------------------
def squeeze_points(block):
    """count() (cpprcoder.h:543-571) for a block of at most 2^24 bytes -> (the indices of the symbols in front of which every
    non-zero count became (c >> 1) | 1, the 256 final counts)."""
    block = np.ascontiguousarray(block, np.uint8)
    assert len(block) <= 1 << 24
    order = np.argsort(block, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(block, minlength=256))])
    counts = np.zeros(256, np.int64)
    at, points = 0, []
    while True:
        first = len(block)
        for v in range(256):  # the occurrence of v in front of which its count is 0xFFFF
            pos = order[starts[v]: starts[v + 1]]
            k = int(np.searchsorted(pos, at)) + 0xFFFF - int(counts[v])
            if k < len(pos):
                first = min(first, int(pos[k]))
        counts += np.bincount(block[at:first], minlength=256)
        if first == len(block):
            return points, counts.astype(np.uint32)
        points.append(first)
        counts = np.where(counts > 0, (counts >> 1) | 1, 0)
        counts[block[first]] += 1
        at = first + 1


def _fillers(rs, n):
    """n bytes other than DOMINANT, spread over all of them (no other count comes near 0xFFFF)."""
    others = np.array([v for v in range(256) if v != DOMINANT], np.uint8)
    return others[rs.randint(0, 255, n)]


def _dominated(rs, n, where_not):
    """n bytes DOMINANT but at the indices where_not, which get fillers."""
    d = np.full(n, DOMINANT, np.uint8)
    d[where_not] = _fillers(rs, len(where_not))
    return d


def _squeeze_at(rs, p, n=LADDER_BLOCK, in_piece=False):
    """A block whose 65536th DOMINANT is at index p: 65535 of them and p - 65535 fillers in front of it, a seeded mix behind
    it.  in_piece: the fillers sit right in front of p (all but one, when p >= 65536), so that the 16-byte piece around p
    holds other symbols in front of p; behind p it holds fillers and DOMINANT again either way."""
    nfill = p - 65535
    if in_piece and nfill > 1:
        where = np.concatenate([rs.choice(65520, 1), np.arange(p - (nfill - 1), p)])
    else:
        where = rs.choice(min(p, 65520), nfill, replace=False)
    head = _dominated(rs, p, where)
    tail = np.where(rs.randint(0, 2, n - p - 1) == 1, np.uint8(DOMINANT), _fillers(rs, n - p - 1)).astype(np.uint8)
    return np.concatenate([head, [np.uint8(DOMINANT)], tail])


def _count_of(rs, mx, more, n=LADDER_BLOCK):
    """A block with mx DOMINANT among its first EASY16 symbols and `more` behind them, at seeded places."""
    head = _dominated(rs, EASY16, rs.choice(EASY16, EASY16 - mx, replace=False))
    tail = _dominated(rs, n - EASY16, rs.choice(n - EASY16, n - EASY16 - more, replace=False))
    return np.concatenate([head, tail])


@functools.lru_cache(maxsize=None)
def squeeze_ladder():
    """-> ([(name, block, the indices where count() squeezes)] of LADDER_BLOCK bytes each, the one block of 131072 bytes
    with two squeezes).  The list has 64 entries, one wave of the encoders at 64 blocks a workgroup: blocks that squeeze in
    different pieces, the two of p = 65543 (and the two of the last symbol) in the same piece, blocks that never squeeze,
    and calm ones (largest count over the first EASY16 symbols + the symbols left < 0xFFFF) among them, so that the wave as
    a whole is not calm; taken alone (one block a workgroup, as the default launch has it for so few blocks) each block
    is on its own side of `calm`."""
    rs = np.random.RandomState(77)
    left = LADDER_BLOCK - EASY16  # 1040
    out = [("p=65535", _squeeze_at(rs, 65535), [65535])]
    for s in range(16):
        p = 65536 + s
        out.append((f"p={p}", _squeeze_at(rs, p, in_piece=bool(s & 1)), [p]))
    out.append(("p=65543 again", _squeeze_at(rs, 65543), [65543]))
    out.append(("p=65863", _squeeze_at(rs, 65536 + 16 * 20 + 7, in_piece=True), [65863]))
    out.append(("p=66559", _squeeze_at(rs, LADDER_BLOCK - 1), [LADDER_BLOCK - 1]))
    # no squeeze: the dominant count ends at 0xFFFE and at 0xFFFF
    out.append(("ends at 0xFFFE", _count_of(rs, EASY16 - 3, 0xFFFE - (EASY16 - 3)), []))
    out.append(("ends at 0xFFFF", _count_of(rs, EASY16 - 3, 0xFFFF - (EASY16 - 3)), []))
    # around `calm`: the largest count so far + the symbols left = 0xFFFE (calm), 0xFFFF (not calm, no squeeze possible),
    # 0x10000 (not calm; every symbol left is DOMINANT, so the last one is squeezed in front of)
    out.append(("calm 0xFFFE", _count_of(rs, 0xFFFE - left, left), []))
    out.append(("calm 0xFFFF", _count_of(rs, 0xFFFF - left, left), []))
    out.append(("calm 0x10000", _count_of(rs, 0x10000 - left, left), [LADDER_BLOCK - 1]))
    while len(out) < 64:  # calm blocks and squeezes at seeded places, alternating
        k = len(out)
        if k & 1:
            out.append((f"calm {k}", _count_of(rs, int(rs.randint(0, 60000)), int(rs.randint(0, left + 1))), []))
        else:
            p = int(rs.randint(65552, LADDER_BLOCK))
            out.append((f"p={p} ({k})", _squeeze_at(rs, p, in_piece=bool(k & 2)), [p]))
    # two squeezes: the 65536th DOMINANT, and, its count halved to 32768 by then, the 32768th behind that
    n2 = 131072
    twice = _dominated(rs, n2, rs.choice(n2 - 16, n2 - (65536 + 32768 + 2000), replace=False))
    return out, twice


def ladder_bytes():
    return np.concatenate([b for _, b, _ in squeeze_ladder()[0]])


# ---- the two natural inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def natural_block():
    """16 647 552 bytes, byte i exactly NEAR_FLAT[i] times, in seeded order: count() never squeezes (no count is 0xFFFF in
    front of an increment), so the block's own table is NEAR_FLAT, the largest total a block reaches without a squeeze
    short of the flat table."""
    return np.random.RandomState(5).permutation(np.repeat(np.arange(256, dtype=np.uint8), NEAR_FLAT))


@functools.lru_cache(maxsize=None)
def natural_stream():
    """2^24 bytes: longer than RCX_MAX_BLOCK = 2^24 - 256, so a single stream that the one-lane kernels code, and not longer
    than 2^24, so count()'s second rescale (cpprcoder.h:561-570) stays out.  65536 x DOMINANT first: one squeeze, in front of
    the last of them, which leaves DOMINANT at 32768; behind that, in seeded order, 32767 more of DOMINANT and 65407 or
    65408 of every other byte, so no count is 0xFFFF in front of an increment again.  Total 2^24 - 32768."""
    rest = np.full(256, 65407, np.int64)
    rest[np.array([v for v in range(256) if v != DOMINANT])[:128]] += 1
    rest[DOMINANT] = 32767
    assert int(rest.sum()) == (1 << 24) - 65536
    tail = np.random.RandomState(6).permutation(np.repeat(np.arange(256, dtype=np.uint8), rest))
    return np.concatenate([np.full(65536, DOMINANT, np.uint8), tail])
