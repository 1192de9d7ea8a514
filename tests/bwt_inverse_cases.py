"""Inputs for the inverse block sort (csrc/rcx_bwt.hpp, rcx_bwt_inv_k) at the points where it changes path, and the
model that aims them.  BlkSort::decode (blksort.h:543-679) is defined for any column and any row below 32768: `next` is
the stable argsort of the column and the output is a walk along it, so a column can be written down whose walk has the
pieces, marks, links and cycle a test wants, and whose batches of 64 keys put the counting pass (rcx_bwt_pass) on either
side of its pile switch.

inverse_walk and pile_plan are MODELS read from the kernel's code, not measurements -- the kernel reports none of these
quantities -- and not a source of expected bytes: those come from the oracle.  tests/test_bwt_inverse_cases_cpu.py holds
the model to the oracle and asserts every figure a case is named for; tests/test_gpu_bwt_inverse.py runs the blocks.

A block here is the 32770 encoded bytes: the column, then the row (little-endian).  Everything is integer arithmetic.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import bwt_cases
from bwt_cases import BLOCK, ENCODED

PIECES = 1024     # the walk is cut at the rows congruent to next[row] modulo 32: one piece per thread
STRETCH = 32      # rows between two marks, and the most that one job of the second walk writes
ROUNDS = 10       # of pointer jumping: 2^10 = PIECES
MARKS_BOUND = 992  # sum over the pieces of (length - 1) // 32 with 1024 pieces of >= 1 row and 32768 rows in all
PILE = 32         # RCX_BWT_PILE: more lanes than this on one digit in a sampled batch and the group of 8 is matched
WAVES, BATCH, GROUP = 16, 64, 8   # the inverse pass: 16 waves x 32 batches of 64 keys, every 8th sampled


def block(column, row: int) -> np.ndarray:
    col = np.asarray(column)
    assert col.shape == (BLOCK,) and 0 <= row < BLOCK and int(col.min()) >= 0 and int(col.max()) <= 255
    return np.concatenate([col.astype(np.uint8), np.array([row & 0xFF, row >> 8], np.uint8)])


def split(blk: np.ndarray) -> tuple[np.ndarray, int]:
    assert len(blk) == ENCODED
    return blk[:BLOCK], int(blk[BLOCK]) | int(blk[BLOCK + 1]) << 8


@dataclass
class Walk:
    next: np.ndarray       # the stable argsort of the column
    residue: int           # next[row] & 31
    first: int             # next[row] >> 5: the piece the walk starts with, made a sink
    lens: np.ndarray       # rows of each of the 1024 pieces (`lens`)
    into: np.ndarray       # the piece each runs into ((r >> 5) where its walk broke off)
    piece_marks: np.ndarray  # marks each piece notes
    marks: int             # misc[40]
    cycle: int             # misc[41], by the kernel's formula from the jumped links
    on_walk: np.ndarray    # bool per piece: v == first or (link[v] >> 16) == first after the jumping
    on: int                # how many of them
    off_marks: int         # marks that belong to pieces off the walk: job 1 must refuse them
    link: np.ndarray       # link << 16 | distance of every piece after the jumping

    @property
    def longest(self) -> int:
        return int(self.lens.max())


def inverse_walk(column, row: int, rounds: int = ROUNDS) -> Walk:
    """What rcx_bwt_inv_k computes on the way for this column and row.  The first walk: thread v goes from row
    residue + 32 v along next until it meets a row congruent to residue (the break comes BEFORE the mark test, so a piece
    of exactly 32 rows notes nothing: a piece of n rows notes (n - 1) // 32 marks).  Then `rounds` rounds of pointer
    jumping on link << 16 | distance with 16 bits of distance, the first piece a sink, and the kernel's formula for the
    cycle.  (Vectorised: the first walk by doubling over the rows.)"""
    col = np.asarray(column, np.uint8)
    assert col.shape == (BLOCK,) and 0 <= row < BLOCK
    nxt = np.argsort(col, kind="stable").astype(np.int64)
    x0 = int(nxt[row])
    residue, first = x0 & 31, x0 >> 5
    is_start = (np.arange(BLOCK) & 31) == residue
    # tgt[r], dist[r]: where the walk from r stands after dist[r] steps, stopped at the first start it meets
    tgt, dist = nxt.copy(), np.ones(BLOCK, np.int64)
    for _ in range(15):     # 2^15 steps: more than the longest piece there can be
        act = np.nonzero(~is_start[tgt])[0]
        if not len(act):
            break
        t = tgt[act]
        dist[act] += dist[t]
        tgt[act] = tgt[t]
    starts = residue + 32 * np.arange(PIECES)
    assert is_start[tgt[starts]].all()      # a permutation comes back to its start
    lens, into = dist[starts], tgt[starts] >> 5
    piece_marks = (lens - 1) // STRETCH
    word = (into << 16) | lens
    word[first] = first << 16
    for _ in range(rounds):
        there = word[word >> 16]
        word = (there & 0xFFFF0000) | ((word + there) & 0xFFFF)
    r5 = int(into[first])
    cycle = int(lens[first]) + (0 if r5 == first else int(word[r5]) & 0xFFFF)
    on_walk = (word >> 16) == first
    on_walk[first] = True
    return Walk(nxt, residue, first, lens, into, piece_marks, int(piece_marks.sum()), cycle, on_walk, int(on_walk.sum()),
                int(piece_marks[~on_walk].sum()), word)


def stray_bytes(walk: Walk) -> int:
    """How many bytes job 1 would put inside the output for stretches of pieces OFF the walk if it did not refuse them
    (position cycle - distance + skip, with whatever the jumping left as the distance of such a piece: mostly that is
    past the block's end, and the refusal shows only in blocks where it is not)."""
    total = 0
    for v in np.nonzero(~walk.on_walk & (walk.piece_marks > 0))[0]:
        for k in range(1, int(walk.piece_marks[v]) + 1):
            at = (walk.cycle - (int(walk.link[v]) & 0xFFFF) + STRETCH * k) & 0xFFFFFFFF
            total += max(0, min(int(walk.lens[v]) - STRETCH * k, STRETCH, BLOCK - at))
    return total


def serial_rows(nxt: np.ndarray, row: int) -> np.ndarray:
    """next[row], next[next[row]], ...: the 32768 rows the reference's walk reads, by doubling."""
    rows = np.empty(BLOCK, np.int64)
    rows[0] = nxt[row]
    jump, have = nxt, 1
    while have < BLOCK:
        rows[have: 2 * have] = jump[rows[:have]]
        jump = jump[jump]
        have *= 2
    return rows


def laid_out(column, row: int, walk: Walk) -> np.ndarray:
    """The model's output: the bytes of the first `cycle` rows of the serial walk, each at position + m * cycle."""
    col = np.asarray(column, np.uint8)
    return np.resize(col[serial_rows(walk.next, row)[: walk.cycle]], BLOCK)


def pile_plan(column, pile: int = PILE) -> np.ndarray:
    """bool[wave][group of 8 batches]: whether the inverse's counting pass matches the group (True: some digit has more
    than `pile` lanes in the sampled batch, the group's first) or counts its other seven batches with the LDS atomic.
    Batch `it` of wave w is column[2048 w + 64 it .. + 64): the pass starts from the identity."""
    col = np.asarray(column, np.uint8)[:BLOCK].reshape(WAVES, BLOCK // (WAVES * BATCH * GROUP), GROUP, BATCH)
    plan = np.zeros(col.shape[:2], bool)
    for w in range(col.shape[0]):
        for g in range(col.shape[1]):
            plan[w, g] = int(np.bincount(col[w, g, 0], minlength=256).max()) > pile
    return plan


# ---- the walk families ------------------------------------------------------------------------------------------------
def descent(C: int, lead: int) -> np.ndarray:
    """0^lead, then 2, 3, ..., C, 1, then C + 1 to the end; row `lead`.  Rows lead .. lead + C - 1 are one cycle of C rows
    (lead -> lead + C - 1 -> lead + C - 2 -> ...), every other row is a fixed point."""
    assert 1 <= C <= 254 and lead + C <= BLOCK
    col = np.full(BLOCK, C + 1, np.int64)
    col[:lead] = 0
    col[lead: lead + C] = np.concatenate([np.arange(2, C + 1), [1]])
    return block(col, lead)


def rotation(M: int, s: int, lead: int = 0) -> np.ndarray:
    """0^lead 2^s 1^(M - s) 3^rest, row `lead`: rows lead .. lead + M - 1 turn by s, in cycles of M / gcd(M, s)."""
    assert 0 < s < M and lead + M <= BLOCK
    col = np.full(BLOCK, 3, np.int64)
    col[:lead] = 0
    col[lead: lead + s] = 2
    col[lead + s: lead + M] = 1
    return block(col, lead)


def steps3(a: int, b: int) -> np.ndarray:
    """2^a 1^b 0^rest, row 0: an exchange of three intervals."""
    assert a > 0 and b > 0 and a + b < BLOCK
    col = np.zeros(BLOCK, np.int64)
    col[:a] = 2
    col[a: a + b] = 1
    return block(col, 0)


def modulo(k: int, row: int) -> np.ndarray:
    return block(np.arange(BLOCK) % k, row)


def exact_32() -> np.ndarray:
    """The column of the text 0^(N-1) 1: next is r -> r + 1, and every piece has exactly 32 rows."""
    col = np.zeros(BLOCK, np.int64)
    col[0] = 1
    return block(col, 0)


# What each case is named for: the model's figures (inverse_walk), asserted by the CPU test.  "longest": the longest piece,
# "lens": the set of piece lengths, "self": the first piece runs into itself (the `(r >> 5) == first` term).
DESCENT_ON = {1: 1, 2: 1, 31: 1, 32: 1, 33: 2, 63: 2, 64: 2, 65: 3, 254: 8}
DESCENT = [(C, lead) for C in DESCENT_ON for lead in (0, 17)] + [
    (33, BLOCK - 33),    # next[row] = 32767: first 1023, residue 31
    (2, BLOCK - 33),     # next[row] = 32736: first 1023, residue 0
    (254, 32 * 1023 - 253 + 31 - 32)]  # a cycle of 8 pieces that ends in the last but one piece
ROTATION = {
    (1023, 1, 0): dict(cycle=1023, on=32),
    (1025, 1, 0): dict(cycle=1025, longest=33, marks=1),
    (32767, 1, 0): dict(cycle=32767, on=1024, lens={31, 32}, marks=0),
    (32767, 2, 0): dict(cycle=32767, longest=16399, marks=512),
    (32767, 32, 0): dict(cycle=32767, longest=31744, marks=991),
    (32767, 31, 0): dict(cycle=1057, on=33),
    (32736, 1, 0): dict(cycle=32736, on=1023),
    (2048, 33, 0): dict(cycle=2048, on=64),
    (16384, 1, 0): dict(cycle=16384, on=512),
    (16416, 1, 0): dict(cycle=16416, on=513),
    (16448, 1, 0): dict(cycle=16448, on=514),
    (16384, 1, 5): dict(cycle=16384, on=512),
    (16448, 1, 5): dict(cycle=16448, on=514),
}
STEPS3 = {
    (1, 31): dict(cycle=32768, on=1024, longest=31745, marks=992),
    (1, 1): dict(cycle=32768, longest=16400, marks=512),
    (2, 2): dict(cycle=16384, on=1024, longest=8200),
    (2, 1): dict(cycle=10923, on=342),
    (3, 2): dict(cycle=6554, on=205),
    (32, 1): dict(cycle=993, on=31, marks=31),
    (32, 16384): dict(cycle=342, on=342, lens={1}),
    (32, 32): dict(cycle=1024, lens={1}),
    (16383, 2): dict(cycle=2),
}
MODULO = [(5, 0), (7, 0), (100, 0), (255, 0),          # row 0 is a fixed point; hundreds of marks lie off the walk
          (5, 1), (7, 3), (100, 99), (255, 254), (255, 129), (3, 32767),
          (39, 31), (10, 5000), (18, 33), (35, 1000)]   # stretches off the walk that would land INSIDE the output (MODULO_STRAY)
MODULO_STRAY = {(39, 31): 629, (10, 5000): 562, (18, 33): 561, (35, 1000): 554}   # stray_bytes(): what refusing them keeps out


def walk_cases() -> dict[str, list[tuple[str, np.ndarray]]]:
    """family -> [(name with the parameters, block)]"""
    return {
        "descent": [(f"descent(C={C}, lead={lead})", descent(C, lead)) for C, lead in DESCENT],
        "rotation": [(f"rotation(M={M}, s={s}, lead={lead})", rotation(M, s, lead)) for M, s, lead in ROTATION],
        "steps3": [(f"steps3(a={a}, b={b})", steps3(a, b)) for a, b in STEPS3],
        "modulo": [(f"modulo(k={k}, row={row})", modulo(k, row)) for k, row in MODULO],
        "exact_32": [("exact_32()", exact_32())],
    }


# ---- the counting pass's pile switch -----------------------------------------------------------------------------------
def by_batch(fill) -> np.ndarray:
    """A column from fill(wave, batch) -> 64 digits, laid where the inverse pass reads them."""
    col = np.empty(BLOCK, np.int64)
    for w in range(WAVES):
        for it in range(BLOCK // (WAVES * BATCH)):
            at = 2048 * w + BATCH * it
            col[at: at + BATCH] = fill(w, it)
    return col


def _sampled(digit: int, lanes: int, turn: int = 0) -> np.ndarray:
    """A batch with `lanes` lanes on `digit` and every other lane on a digit of its own, turned by `turn` lanes."""
    others = (digit + 1 + np.arange(BATCH - lanes)) % 256
    return np.roll(np.concatenate([np.full(lanes, digit, np.int64), others]), turn)


def pile_digit(digit: int, lanes: int) -> np.ndarray:
    """Every sampled batch: `lanes` lanes on `digit`, the others all different; the seven behind it: all 64 on `digit`.
    With 64 lanes there are no others: every batch is then wholly on `digit` or on `digit + 2` (the same half of another
    dword), in an order that leaves cycles of hundreds of rows rather than the identity."""
    if lanes == BATCH:
        return by_batch(lambda w, it: np.full(BATCH, digit + 2 * ((it * 7 + w * 3) % 5 % 2)))
    return by_batch(lambda w, it: _sampled(digit, lanes, 3 * w + it) if it % GROUP == 0 else np.full(BATCH, digit))


def pile_pair(k: int, lanes_alternate: bool) -> np.ndarray:
    """Digits 2k and 2k + 1, the two halves of one dword of counts.  Sampled batches: 32 lanes on 2k + 1 (not piled).
    The seven behind: all 64 lanes on 2k, so that the lower half takes 7 x 64 x 4 = 1792 atomic adds in a wave next to
    matched 16-bit writes of the upper half -- or, `lanes_alternate`, even lanes on 2k and odd lanes on 2k + 1: one
    instruction adds to both halves."""
    lanes = 2 * k + (np.arange(BATCH) & 1)
    return by_batch(lambda w, it: _sampled(2 * k + 1, 32, w + it) if it % GROUP == 0 else (lanes if lanes_alternate else np.full(BATCH, 2 * k)))


def pile_by_wave() -> np.ndarray:
    """Wave w's group g is piled unless bit g of w is set: wave 0 in every group, wave 15 in none, every mixture
    between.  Piled groups sample 64 lanes of one digit, the others 64 different digits; the batches behind are
    pseudo-random digits from a small alphabet, so that the waves' counts of one digit meet in the prefix."""
    noise = bwt_cases.mix(BLOCK, 4100).astype(np.int64) % 12

    def fill(w, it):
        if it % GROUP:
            return 100 + noise[2048 * w + BATCH * it: 2048 * w + BATCH * (it + 1)]
        return np.full(BATCH, 100 + (w + it // GROUP) % 12) if not (w >> (it // GROUP)) & 1 else (90 + np.arange(BATCH))
    return by_batch(fill)


def spread_rows(column, want: int = 4) -> list[int]:
    """Rows on the `want` longest cycles of the column's permutation (the output shows `next` only along the walk);
    of the fixed points only one."""
    nxt = np.argsort(np.asarray(column, np.uint8), kind="stable")
    seen, found = np.zeros(BLOCK, bool), []
    for r in range(BLOCK):
        if not seen[r]:
            n, p = 0, r
            while not seen[p]:
                seen[p] = True
                p = int(nxt[p])
                n += 1
            found.append((-n, r))
    found.sort()
    return [r for i, (n, r) in enumerate(found[:want]) if i == 0 or n < -1]


def pile_columns() -> list[tuple[str, np.ndarray, str]]:
    """[(name, column, plan)]: plan is "none", "all" or "by wave" -- what pile_plan must say."""
    out = []
    for digit in (6, 201):                       # an even and an odd digit: either half of the dword
        for lanes in (32, 33, 64):
            out.append((f"digit {digit}, {lanes} lanes sampled", pile_digit(digit, lanes), "none" if lanes <= PILE else "all"))
    out.append(("pair 2k / 2k + 1, lower half piled by atomics", pile_pair(40, False), "none"))
    out.append(("pair 2k / 2k + 1, lanes alternate", pile_pair(40, True), "none"))
    out.append(("waves differ", pile_by_wave(), "by wave"))
    one = np.zeros(BLOCK, np.int64)
    for name, at, a, b in (("first, smaller", 0, 0, 1), ("last, smaller", BLOCK - 1, 0, 1), ("first, larger", 0, 1, 0),
                           ("last, larger", BLOCK - 1, 1, 0)):
        col = one + b
        col[at] = a
        out.append((f"32767 of one digit and one of another ({name})", col, "all"))
    e = np.arange(BLOCK)
    out.append(("256 digits x 128, a new digit every lane", (e + (e >> 8) * 37) & 255, "none"))   # (e % 256 is modulo(256, .): cycles of 15)
    out.append(("256 digits x 128, in runs", ((e // 128) * 37 + 11) % 256, "all"))                # (sorted runs are the identity)
    out.append(("digit 255 only", np.full(BLOCK, 255, np.int64), "all"))
    return out


def pile_cases() -> list[tuple[str, np.ndarray]]:
    """Every pile column with rows on its longest cycles."""
    return [(f"{name}, row {row}", block(col, row)) for name, col, _ in pile_columns() for row in spread_rows(col)]


def all_cases() -> dict[str, list[tuple[str, np.ndarray]]]:
    c = walk_cases()
    c["pile"] = pile_cases()
    return c
