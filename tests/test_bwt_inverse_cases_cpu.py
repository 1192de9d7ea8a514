"""What tests/test_gpu_bwt_inverse.py takes for granted about the blocks tests/bwt_inverse_cases.py builds for the inverse
block sort (csrc/rcx_bwt.hpp, rcx_bwt_inv_k and the counting pass rcx_bwt_pass under it), checked without a GPU: every
block has the pieces, marks, links and cycle it is named for, and every pile column puts each wave's groups of batches
on the side of the pile switch it is meant to.

bwt_inverse_cases.inverse_walk and pile_plan are models of the kernel, derived from its code, not measured: the kernel
reports none of these quantities.  The model is held here to the definition (the serial walk along the stable argsort)
and, laid out as position + m * cycle, to the oracle's inverse."""
from math import gcd

import numpy as np
import pytest

import bwt_inverse_cases as ic
from bwt_cases import BLOCK, ENCODED


@pytest.fixture(scope="module")
def built():
    """family -> [(name, block, the model's walk)], made once."""
    return {family: [(name, blk, ic.inverse_walk(*ic.split(blk))) for name, blk in items] for family, items in ic.all_cases().items()}


def every(built):
    return [(family, *item) for family, items in built.items() for item in items]


def by_name(built, family):
    return {name: walk for name, _, walk in built[family]}


def check_figures(walk, want, name):
    for key, value in want.items():
        got = set(walk.lens.tolist()) if key == "lens" else getattr(walk, key)
        assert got == value, (name, key, got, value)


def test_every_block_is_a_block_the_reference_can_walk(built):
    names = [name for _, name, _, _ in every(built)]
    assert len(names) == len(set(names)) and 100 <= len(names) <= 150
    for _, name, blk, _ in every(built):
        assert blk.dtype == np.uint8 and len(blk) == ENCODED, name
        assert ic.split(blk)[1] < BLOCK, name        # the reference reads inside its arrays (blksort.h:663)


def test_the_model_is_the_serial_walk(built):
    """The definition, without pieces: follow next from next[row] until it comes back.  The model's cycle (the kernel's
    formula over the jumped links), its pieces on the walk and their lengths must be that walk's; the pieces partition
    the rows of the cycles that hold a start row, so their lengths sum to the number of those rows -- 32768 where every
    cycle of the permutation holds one, fewer where it has cycles (fixed points mostly) that no piece enters."""
    whole = 0
    for _, name, blk, walk in every(built):
        col, row = ic.split(blk)
        assert np.array_equal(np.sort(walk.next), np.arange(BLOCK)) and np.array_equal(col[walk.next], np.sort(col)), name
        assert (np.diff(walk.next)[np.diff(col[walk.next].astype(int)) == 0] > 0).all(), name     # equal bytes in their order
        rows = ic.serial_rows(walk.next, row)
        assert rows[0] == walk.next[row] == walk.residue + 32 * walk.first, name
        back = np.nonzero(rows[1:] == rows[0])[0]
        cycle = int(back[0]) + 1 if len(back) else BLOCK
        assert walk.cycle == cycle, name
        on = np.nonzero((rows[:cycle] & 31) == walk.residue)[0]           # the steps at which the walk stands on a start row
        assert walk.on == len(on) and sorted(np.nonzero(walk.on_walk)[0]) == sorted(rows[on] >> 5), name
        assert np.array_equal(walk.lens[rows[on] >> 5], np.diff(np.concatenate([on, [cycle]]))), name
        assert np.array_equal(walk.into[rows[on] >> 5], np.roll(rows[on] >> 5, -1)), name
        # the rows of all the pieces: walk every start's cycle
        reached = np.zeros(BLOCK, bool)
        for v in range(ic.PIECES):
            p = walk.residue + 32 * v
            while not reached[p]:
                reached[p] = True
                p = int(walk.next[p])
        assert int(walk.lens.sum()) == int(reached.sum()) <= BLOCK, name
        assert walk.lens.min() >= 1 and np.array_equal(walk.piece_marks, (walk.lens - 1) // 32), name
        whole += int(reached.all())
    assert whole >= 5           # (blocks whose pieces do hold all 32768 rows: steps3(1, 31), steps3(1, 1), exact_32 and more)


def test_marks_stay_within_their_bound_and_one_block_reaches_it(built):
    """mark_row and mark_of have 1024 entries; 1024 pieces of at least one row and 32768 rows in all leave at most
    (32768 - 1024) / 32 = 992 marks.  steps3(1, 31) has them: one piece of 31 745 rows."""
    most = {name: walk.marks for _, name, _, walk in every(built)}
    assert max(most.values()) == ic.MARKS_BOUND == (BLOCK - ic.PIECES) // 32
    assert most["steps3(a=1, b=31)"] == 992 and by_name(built, "steps3")["steps3(a=1, b=31)"].longest == 31745


def test_the_models_walk_laid_out_by_its_cycle_is_the_oracles_inverse(oracle, built):
    items = every(built)
    want = oracle.bwt_decode(np.concatenate([blk for _, _, blk, _ in items]), threads=4)
    for i, (_, name, blk, walk) in enumerate(items):
        assert np.array_equal(ic.laid_out(*ic.split(blk), walk), want[i * BLOCK:(i + 1) * BLOCK]), name


def test_descent_is_one_cycle_of_C_rows(built):
    walks = by_name(built, "descent")
    assert len(walks) == len(ic.DESCENT) == 21
    ends = set()
    for C, lead in ic.DESCENT:
        walk = walks[f"descent(C={C}, lead={lead})"]
        where = lead + C - 1                      # next[row]
        assert (walk.cycle, walk.on, walk.marks) == (C, ic.DESCENT_ON[C], 0), (C, lead)
        assert (walk.first, walk.residue) == (where >> 5, where & 31), (C, lead)
        assert (walk.into[walk.first] == walk.first) == (C <= 32), (C, lead)      # the `(r >> 5) == first` term
        assert C > 32 or walk.lens[walk.first] == C, (C, lead)
        ends.add((walk.first, walk.residue))
    assert ic.DESCENT_ON == {1: 1, 2: 1, 31: 1, 32: 1, 33: 2, 63: 2, 64: 2, 65: 3, 254: 8}
    assert {(0, 0), (0, 31), (1023, 0), (1023, 31)} <= ends
    assert {w.residue for w in walks.values()} >= {0, 31} and {w.first for w in walks.values()} >= {0, 1023}


def test_rotation_has_the_figures_it_is_named_for(built):
    walks = by_name(built, "rotation")
    for (M, s, lead), want in ic.ROTATION.items():
        walk = walks[f"rotation(M={M}, s={s}, lead={lead})"]
        assert walk.cycle == M // gcd(M, s), (M, s)
        check_figures(walk, want, (M, s, lead))
    assert walks["rotation(M=1025, s=1, lead=0)"].lens.tolist().count(33) == 1      # one piece of 33 rows, one mark
    assert 31 in walks["rotation(M=32767, s=1, lead=0)"].lens
    assert [walks[f"rotation(M={M}, s=1, lead=0)"].on for M in (16384, 16416, 16448, 32736, 32767)] == [512, 513, 514, 1023, 1024]
    assert ic.ROTATION[(32767, 31, 0)]["cycle"] == 1057 and 32768 % 1057 and 32768 % 32767 and 32768 % 1023


def test_steps3_has_the_figures_it_is_named_for(built):
    walks = by_name(built, "steps3")
    for (a, b), want in ic.STEPS3.items():
        check_figures(walks[f"steps3(a={a}, b={b})"], want, (a, b))
    laps = walks["steps3(a=2, b=2)"]
    assert 2 * laps.cycle == BLOCK and laps.on == 1024            # exactly two laps, every piece on the walk
    few = walks["steps3(a=32, b=1)"]
    assert (few.marks, few.off_marks) == (31, 30)                  # most of the marks lie off the walk
    assert walks["steps3(a=32, b=32)"].on == 1024 and walks["steps3(a=16383, b=2)"].on == 1


def test_modulo_leaves_hundreds_of_marks_off_the_walk(built):
    walks = by_name(built, "modulo")
    off = {}
    for k, row in ic.MODULO:
        walk = walks[f"modulo(k={k}, row={row})"]
        if row == 0:      # a fixed point: every stretch job 1 is handed must be refused
            assert (walk.cycle, walk.on) == (1, 1) and walk.off_marks == walk.marks, k
            off[k] = walk.marks
        else:
            assert walk.cycle > 32 and walk.on > 1, (k, row)      # a longer cycle: stretches taken and, k = 3 apart, refused
            assert walk.off_marks > 0 or k == 3, (k, row)
    assert off == {5: 626, 7: 616, 100: 589, 255: 565}
    cycles = {(k, row): walks[f"modulo(k={k}, row={row})"].cycle for k, row in ic.MODULO if row}
    assert cycles == {(5, 1): 9481, (7, 3): 8434, (100, 99): 13419, (255, 254): 15561, (255, 129): 6101, (3, 32767): 8192,
                      (39, 31): 29972, (10, 5000): 28838, (18, 33): 26097, (35, 1000): 24788}


def test_refusing_the_stretches_off_the_walk_shows_in_the_output(built):
    """A stretch of a piece off the walk would go to cycle - distance + skip, with a distance that the jumping leaves
    meaningless: for most blocks -- every modulo block above with row 0 -- that is past the block's end and nothing would be
    written even without the `(there >> 16) == first` test.  The MODULO_STRAY blocks are the ones where hundreds of such
    bytes would land inside the output."""
    walks = by_name(built, "modulo")
    for k, row in ic.MODULO:
        stray = ic.stray_bytes(walks[f"modulo(k={k}, row={row})"])
        assert stray == ic.MODULO_STRAY.get((k, row), 0), (k, row, stray)
    assert len(ic.MODULO_STRAY) == 4 and min(ic.MODULO_STRAY.values()) > 500
    assert all(ic.stray_bytes(walk) == 0 for _, _, _, walk in every(built) if walk.off_marks == 0)


def test_exact_32_is_1024_pieces_of_32_rows(built):
    (_, _, walk), = built["exact_32"]
    assert set(walk.lens.tolist()) == {32} and (walk.marks, walk.cycle, walk.on) == (0, BLOCK, 1024)   # break and mark on one step: the break wins


def test_the_edges_named_are_all_there(built):
    walks = [walk for _, _, _, walk in every(built)]
    assert {1, 2, 512, 513, 514, 1023, 1024} <= {w.on for w in walks}
    assert {1, 2, 31, 32, 33, 32767, 32768} <= {w.cycle for w in walks}
    assert {31, 32, 33, 31745} <= {int(n) for w in walks for n in np.unique(w.lens)}
    assert any(w.off_marks and w.off_marks < w.marks for w in walks)       # refused and accepted stretches in one block
    assert any(w.cycle < 32 and w.marks > 500 for w in walks) and any(w.cycle == BLOCK and w.marks == 0 for w in walks)


def test_nine_rounds_of_jumping_serve_up_to_513_pieces_on_the_walk(built):
    """k rounds carry a link 2^k pieces along the walk; the farthest piece is on - 1 links from the first, and the cycle is
    read from the piece behind the first, which is that one.  So 9 rounds give the same cycle and the same pieces on the
    walk up to on = 513, and from 514 on the tenth is needed: the blocks are on both sides."""
    ons = set()
    for _, name, blk, walk in every(built):
        nine = ic.inverse_walk(*ic.split(blk), rounds=9)
        same = nine.cycle == walk.cycle and np.array_equal(nine.on_walk, walk.on_walk)
        assert same == (walk.on <= 513), (name, walk.on)
        ons.add(walk.on)
    assert {512, 513, 514} <= ons


def test_pile_plan_on_small_batches():
    col = np.arange(BLOCK) % 256                         # 64 different digits in every batch
    assert not ic.pile_plan(col).any()
    col[2048 * 3 + 512 * 2: 2048 * 3 + 512 * 2 + 33] = 9   # wave 3, group 2, sampled batch: 33 lanes on 9
    plan = ic.pile_plan(col)
    assert plan[3, 2] and plan.sum() == 1 and plan.shape == (16, 4)
    col[2048 * 3 + 512 * 2] = 10                         # 32 lanes
    assert not ic.pile_plan(col).any() and ic.pile_plan(col, pile=31).sum() == 1
    col[2048 * 3 + 512 * 2 + 64:  2048 * 3 + 512 * 3] = 9  # the seven batches behind are not looked at
    assert not ic.pile_plan(col).any()


def test_every_pile_column_lies_on_the_side_of_the_switch_it_is_meant_to():
    columns = ic.pile_columns()
    assert len(columns) == 16 and {plan for _, _, plan in columns} == {"none", "all", "by wave"}
    by_wave = np.array([[not (w >> g) & 1 for g in range(4)] for w in range(16)])
    assert by_wave[0].all() and not by_wave[15].any() and len({tuple(r) for r in by_wave}) == 16
    for name, col, want in columns:
        plan = ic.pile_plan(col)
        assert plan.shape == (16, 4), name
        assert np.array_equal(plan, {"none": np.zeros((16, 4), bool), "all": np.ones((16, 4), bool), "by wave": by_wave}[want]), name
    cols = {name: np.asarray(col).reshape(16, 4, 8, 64) for name, col, _ in columns}
    for digit in (6, 201):
        for lanes in (32, 33):
            b = cols[f"digit {digit}, {lanes} lanes sampled"]
            assert ((b[:, :, 0] == digit).sum(axis=-1) == lanes).all()                     # exactly 32 against 33 lanes
            for w in range(16):
                for g in range(4):
                    assert np.bincount(b[w, g, 0]).max() == lanes and len(set(b[w, g, 0].tolist())) == 64 - lanes + 1
            assert (b[:, :, 1:] == digit).all()                                            # all 64 lanes on one digit behind
            # one threshold down or up and the column changes sides: what RCX_BWT_PILE = 31 or 33 would move
            assert ic.pile_plan(b.reshape(-1), pile=31).all() and not ic.pile_plan(b.reshape(-1), pile=33).any()
        b = cols[f"digit {digit}, 64 lanes sampled"]
        assert (b == b[..., :1]).all() and set(np.unique(b).tolist()) == {digit, digit + 2}
    low = cols["pair 2k / 2k + 1, lower half piled by atomics"]
    assert ((low == 80).sum(axis=(1, 2, 3)) >= 7 * 64 * 4).all() and ((low[:, :, 1:] == 80).all())   # 1792 adds to the lower half
    assert ((low[:, :, 0] == 81).sum(axis=-1) == 32).all()                                         # beside matched writes of the upper
    alt = cols["pair 2k / 2k + 1, lanes alternate"]
    assert (alt[:, :, 1:, 0::2] == 80).all() and (alt[:, :, 1:, 1::2] == 81).all()
    for name, count in (("first, smaller", 1), ("last, smaller", 1), ("first, larger", 1), ("last, larger", 1)):
        c = cols[f"32767 of one digit and one of another ({name})"].reshape(-1)
        assert sorted(np.bincount(c).tolist()) == [1, 32767]
        assert (c[0] != c[1]) == name.startswith("first") and (c[-1] != c[-2]) == name.startswith("last")
    for name in ("256 digits x 128, a new digit every lane", "256 digits x 128, in runs"):
        assert (np.bincount(cols[name].reshape(-1), minlength=256) == 128).all(), name
    assert (cols["digit 255 only"] == 255).all()


def test_the_pile_rows_lie_on_different_cycles(built):
    """The output shows `next` only along the walk, so every pile column is walked from rows on its longest cycles."""
    seen = {}
    for name, blk, walk in built["pile"]:
        col, row = ic.split(blk)
        rows = set(ic.serial_rows(walk.next, row)[: walk.cycle].tolist())
        key = name.rsplit(", row ", 1)[0]
        assert not (seen.get(key, set()) & rows), name
        seen[key] = seen.get(key, set()) | rows
    assert len(seen) == 16
    for key in ("digit 6, 32 lanes sampled", "digit 201, 33 lanes sampled", "pair 2k / 2k + 1, lower half piled by atomics",
                "pair 2k / 2k + 1, lanes alternate", "waves differ", "256 digits x 128, a new digit every lane"):
        assert len(seen[key]) > BLOCK // 2, (key, len(seen[key]))       # more than half of `next` shows in the output
