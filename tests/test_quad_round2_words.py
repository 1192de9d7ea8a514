"""Round 2 of the adaptive quad decoder (csrc/rcx_quad.hpp, DESIGN 3.4 "Round 7") as integer arithmetic, both ways:

  old   positive counts; the lane's four inclusive sums scaled by t with 24-bit multiply-adds, scanned across the quad
        scaled, subtracted from the remainder in 32 bits; the borrows as carry bits: three counted into the symbol, the
        fourth the owner mask;
  new   negated counts; P = the (negated) counts of the node's symbols in lower lanes from the unscaled sums,
        D = {rem, 0} + P * t and Y_k = Y_(k-1) + l_k * t as signed 64-bit multiply-adds; the low words are the old y, the
        high words the borrows: sym = sb + h_a + h_b + h_c, owner word = ~h_D & h_e.

Every case is one quad (4 lanes x 4 counts = a node's 16 symbols), many cases at once in numpy int64 (a 32 x 32-bit signed
product and five of them summed stay far inside 64 bits).  The two must agree on the symbol, the owning lane, lo, hi and
range, and the new one's high words must be what the safety argument says.  Needs no GPU.
"""
import numpy as np

M = 0xFFFFFFFF
P1, P2, P3 = [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]  # the quad permutations of the DPP steps
M1 = np.array([0, -1, 0, -1], np.int64)  # lane & 1, lane & 2 as masks
M2 = np.array([0, 0, -1, -1], np.int64)
LANE = np.arange(4, dtype=np.int64)


def s32(x):
    """the 32-bit pattern of x as a signed number"""
    return ((x + (1 << 31)) & M) - (1 << 31)


def mul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & M


def quad_min(x):
    return np.repeat(x.min(axis=1)[:, None], 4, axis=1)


def quad_max(x):
    return np.repeat(x.max(axis=1)[:, None], 4, axis=1)


def old_round2(counts, t, rem, node):
    """counts (N, 16) positive, t (N,), rem (N,), node (N,) -> per lane (N, 4): sym, owner flag, lo, hi, range"""
    l = counts.reshape(-1, 4, 4)
    tt = t[:, None]
    qa = mul24(l[:, :, 0], tt)
    qb = (mul24(l[:, :, 1], tt) + qa) & M
    qc = (mul24(l[:, :, 2], tt) + qb) & M
    qe = (mul24(l[:, :, 3], tt) + qc) & M
    tot = (qe + qe[:, P1]) & M
    pre = qe[:, P1] & (M1 & M)
    d2 = (rem[:, None] - pre) & M
    o2 = tot[:, P2] & (M2 & M)
    d2 = (d2 - o2) & M
    ya, yb, yc, ye = (d2 - qa) & M, (d2 - qb) & M, (d2 - qc) & M, (d2 - qe) & M
    c1, c2, c3, own = d2 < qa, d2 < qb, d2 < qc, d2 < qe
    sb = node[:, None] * 16 + 4 * LANE + 3
    sym = (sb - c1 - c2 - c3) & M
    lo = quad_min(np.minimum(np.minimum(d2, ya), np.minimum(yb, yc)))
    hi = quad_max(np.maximum(np.maximum(ya, yb), np.maximum(yc, ye)))
    return sym, own, lo, hi, (lo - hi) & M


def new_pairs(ncounts, t, rem):
    """The five register pairs of the new round 2 as signed 64-bit numbers, (N, 4 lanes, 5): D, Y_a, Y_b, Y_c, Y_e.
    ncounts (N, 16): the words of the row as signed 32-bit numbers (for a node row: the negated counts)."""
    l = ncounts.reshape(-1, 4, 4)
    tt = t[:, None]
    qe = s32(l.sum(axis=2))                       # v_add3_u32, v_add_u32
    pre, o2, o3 = qe[:, P1] & M1, qe[:, P2] & M2, qe[:, P3] & M2
    p = s32(pre + o2 + o3)                        # v_add3_u32
    d = rem[:, None] + p * tt                     # v_mad_i64_i32 on {rem, 0}, which v_mad_u64_u32 rem, 1, 0 made
    ya = d + l[:, :, 0] * tt
    yb = ya + l[:, :, 1] * tt
    yc = yb + l[:, :, 2] * tt
    ye = yc + l[:, :, 3] * tt
    return np.stack([d, ya, yb, yc, ye], axis=2)


def new_round2(ncounts, t, rem, node):
    """-> per lane (N, 4): sym, owner word, lo, hi, range, and the five high words (N, 4, 5): h_D, h_a, h_b, h_c, h_e"""
    y = new_pairs(ncounts, t, rem)
    h, x = y >> 32, y & M
    sb = node[:, None] * 16 + 4 * LANE + 3
    sym = (sb + h[:, :, 1] + h[:, :, 2] + h[:, :, 3]) & M  # v_add3_u32, v_add_u32
    own = (~h[:, :, 0] & h[:, :, 4]) & M                   # v_bfi_b32 h_D, 0, h_e
    lo = quad_min(x[:, :, :4].min(axis=2))
    hi = quad_max(x[:, :, 1:].max(axis=2))
    return sym, own, lo, hi, (lo - hi) & M, h


def t_values(counts):
    """t at 1, at 2^24 - 1 where the block's total allows it, and at the largest value with total * t < 2^32 (the other 15
    nodes hold at least 240 symbols, and a total is at least 256)."""
    total = max(256, int(counts.sum()) + 240)
    tmax = M // total
    return sorted({1, min((1 << 24) - 1, tmax), tmax})


def rem_values(counts, t):
    bounds = [int(c) * t for c in np.cumsum(counts)]
    out = {0, bounds[-1] - 1}
    for b in bounds[:-1]:
        out.update((b, b - 1))
    return sorted(out)


def rows_on_the_edges():
    rows = [np.ones(16, np.int64)]
    for slot in range(16):  # one count at 2^24 - 512 in every slot of every lane
        r = np.ones(16, np.int64)
        r[slot] = (1 << 24) - 512
        rows.append(r)
    rs = np.random.RandomState(7)
    for bits in (2, 6, 12, 18):
        rows.append(rs.randint(1, 1 << bits, 16).astype(np.int64))
    return rows


def valid_cases():
    counts, t, rem = [], [], []
    for r in rows_on_the_edges():
        for tv in t_values(r):
            for v in rem_values(r, tv):
                counts.append(r), t.append(tv), rem.append(v)
    rs = np.random.RandomState(11)
    for _ in range(4000):
        bits = int(rs.randint(1, 21))
        r = rs.randint(1, (1 << bits) + 1, 16).astype(np.int64)
        tmax = M // max(256, int(r.sum()) + 240)
        tv = int(rs.randint(1, tmax + 1)) if rs.randint(2) else tmax
        counts.append(r), t.append(tv), rem.append(int(rs.randint(0, int(r.sum()) * tv)))
    counts, t, rem = np.array(counts, np.int64), np.array(t, np.int64), np.array(rem, np.int64)
    node = np.random.RandomState(13).randint(0, 16, len(t)).astype(np.int64)
    return counts, t, rem, node


def test_the_cases_cover_what_they_should():
    counts, t, rem, _ = valid_cases()
    total = counts.sum(axis=1)
    assert (total * t <= M).all() and (rem < total * t).all() and (t >= 1).all()
    ones = (counts == 1).all(axis=1)
    owner_slot = (np.cumsum(counts, axis=1) * t[:, None] <= rem[:, None]).sum(axis=1)
    assert set(owner_slot[ones]) == set(range(16))          # every owning lane and every slot of it
    assert (t[ones] == (1 << 24) - 1).any() and (t == 1).any()
    big = counts.max(axis=1) == (1 << 24) - 512
    assert set(np.argmax(counts[big], axis=1)) == set(range(16))
    assert set(owner_slot[big]) == set(range(16))
    assert (rem == 0).any() and (rem == total * t - 1).any()


def test_new_round2_equals_the_old_one_on_valid_rows():
    counts, t, rem, node = valid_cases()
    sym0, own0, lo0, hi0, rg0 = old_round2(counts, t, rem, node)
    sym1, own1, lo1, hi1, rg1, h = new_round2(-counts, t, rem, node)
    assert (own0.sum(axis=1) == 1).all()                      # one lane owns the symbol
    assert (own1 == np.where(own0, M, 0)).all()               # the owner word: -1 there, 0 elsewhere
    assert (sym1[own0] == sym0[own0]).all()                   # the symbol, in the lane that owns it
    want = node * 16 + (np.cumsum(counts, axis=1) * t[:, None] <= rem[:, None]).sum(axis=1)
    assert (sym1[own0] == want).all()
    assert (lo1 == lo0).all() and (hi1 == hi0).all() and (rg1 == rg0).all()
    # range = count x t, low = rem - t x the counts below the symbol
    slot = want - node * 16
    below = np.where(np.arange(16)[None, :] < slot[:, None], counts, 0).sum(axis=1)
    assert (lo1[:, 0] == rem - below * t).all()
    assert (rg1[:, 0] == counts[np.arange(len(t)), slot] * t).all()


def test_high_words_on_valid_rows():
    """With a zero-high D -- the owning lane and the lanes below it -- every h_k is 0 or -1; above the owner D is negative,
    h_D is -1 and masks the lane's h_e (-1 or -2) out of the owner word."""
    counts, t, rem, node = valid_cases()
    _, own, _, _, _, h = new_round2(-counts, t, rem, node)
    owner = np.argmax(own == M, axis=1)
    at_or_below = LANE[None, :] <= owner[:, None]
    assert (h[:, :, 0][at_or_below] == 0).all()
    assert np.isin(h[at_or_below], (0, -1)).all()
    assert (h[:, :, 0][~at_or_below] == -1).all()
    assert np.isin(h[~at_or_below], (-1, -2)).all()
    # the high words never fall: a borrow stays a borrow along the lane's chain
    assert (np.diff(h[:, :, 1:], axis=2) <= 0).all()


def arbitrary_cases(n=20000):
    """The scratch row read as counts: any four 32-bit words per lane (parked output bytes often repeat), any remainder,
    any t below 2^24 (a range divided by a total of at least 256)."""
    rs = np.random.RandomState(17)
    words = rs.randint(0, 1 << 32, (n, 16), dtype=np.int64)
    words[: n // 4] = rs.randint(0, 256, (n // 4, 16)) * 0x01010101
    words[n // 4: n // 2] |= 0xFF000000
    words[n // 2: n // 2 + 64] = np.array([0, M, 1 << 31, (1 << 31) - 1], np.int64)[rs.randint(0, 4, (64, 16))]
    t = rs.randint(0, 1 << 24, n, dtype=np.int64)
    t[: 8] = (0, 1, (1 << 24) - 1, (1 << 24) - 1, 0, 1, (1 << 23), (1 << 24) - 1)
    rem = rs.randint(0, 1 << 32, n, dtype=np.int64)
    rem[: 4] = (0, M, 0, M)
    return words, t, rem


def test_pairs_are_true_signed_products_on_arbitrary_words():
    """What the int64 model holds is what v_mad_i64_i32 computes: signed 32 x signed 32 -> 64 added to a 64-bit pair
    modulo 2^64.  Checked against Python's unbounded integers, the lanes' scan done by hand."""
    words, t, rem = arbitrary_cases(3000)
    got = new_pairs(s32(words), t, rem)
    sign64 = lambda v: ((v + (1 << 63)) % (1 << 64)) - (1 << 63)
    sign32 = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)
    for c in range(len(t)):
        w = [sign32(int(v)) for v in words[c]]
        sums = [sign32(sum(w[4 * j: 4 * j + 4])) for j in range(4)]
        for j in range(4):
            p = sign32(sum(sums[:j]))              # the lanes below, as the three masked DPP reads and the add3 give it
            y = sign64(int(rem[c]) + p * int(t[c]))
            want = [y]
            for k in range(4):
                y = sign64(y + w[4 * j + k] * int(t[c]))
                want.append(y)
            assert [int(v) for v in got[c, j]] == want, (c, j)


def test_arbitrary_counts_stay_inside_the_row():
    """The ds_add of the count, formed as the kernel forms it: p_la_ = the lane's base (the block's quarter of its table
    group + 16 x lane) + 256 x node, node = 0 .. 16 from round 1, and the address p_la_ + ((p_sym_ & 3) << 2).  Whatever the
    row holds, it is a dword of the lane's own 16 bytes of the 64-byte row of that node -- for node 16 the scratch row --
    inside the block's quarter of the 17 rows; and the owner word, the operand, is a 32-bit value."""
    GROUP_BYTES, ROW, QUARTER = 4352, 256, 64      # rcx_quad.hpp: RCX_QUAD_GROUP_BYTES, a row, a block's share of it
    words, t, rem = arbitrary_cases()
    n = len(t)
    rs = np.random.RandomState(19)
    node = rs.randint(0, 17, n).astype(np.int64)
    node[: n // 2] = 16
    group, quarter = rs.randint(0, 4, n), rs.randint(0, 4, n)
    mine = group * GROUP_BYTES + quarter * QUARTER               # QuadSeat.mine, as an LDS offset
    leaves = mine[:, None] + 16 * LANE[None, :]                   # QuadSeat.leaves
    sym, own, lo, hi, rg, _ = new_round2(s32(words), t, rem, node)
    p_la = (leaves + (node[:, None] << 8)) & M                    # v_lshl_add_u32 la, nd, 8, lvb
    pad = (((sym & 3) << 2) + p_la) & M                           # v_and_b32 pad, 3, psym; v_lshl_add_u32 pad, pad, 2, pla
    row = mine + ROW * node
    assert (pad % 4 == 0).all()
    assert (pad >= row[:, None] + 16 * LANE[None, :]).all() and (pad + 4 <= row[:, None] + 16 * LANE[None, :] + 16).all()
    assert (pad >= row[:, None]).all() and (pad + 4 <= row[:, None] + QUARTER).all()
    assert (pad + 4 <= (group[:, None] + 1) * GROUP_BYTES).all()  # rows 0 .. 16 of the group: 17 x 256 = its 4352 bytes
    # the symbol did pick every dword of a lane on this input: the assertion above is not about one value
    assert set(np.unique(sym & 3)) == {0, 1, 2, 3}
    assert ((own >> 32) == 0).all() and ((sym >> 32) == 0).all() and ((lo | hi | rg) >> 32 == 0).all()
