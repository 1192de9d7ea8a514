"""Inputs for the rANS kernels' switch points (csrc/rcx_rans.hpp): blocks whose MODEL takes a chosen path through
normalize()'s steal loop, blocks whose coded bytes come as fast as the format allows (the encoders' output rings), and
sets of item lengths that put blocks of chosen lengths side by side in one wave.

Two functions here are MODELS read from the code, for aiming the inputs -- never expected values (expected bytes always
come from the oracle; tests/test_rans_cases_cpu.py holds both models to the oracle):
  normalize_model   cppans.h:138-178 as oracle/rans_oracle.c:46-66 has it, with the steals it makes listed;
  emitted           the two encoders' renormalisation tests, symbol by symbol: what leaves for which symbol.

Everything is built from counts and integer arithmetic; where order does not matter the bytes are shuffled with a fixed
seed.  A builder returns uint8 arrays.
"""
from __future__ import annotations

import numpy as np

BITS = {False: 14, True: 12}   # by the oracle's `simd` flag: the one-state format, the eight-state format
LOSER_BLOCK = 4096 * 17        # 69632 bytes: a count of c scales to c / 17 slots of 4096 and 4 c / 17 of 16384, see victim_cases


# ---- the models --------------------------------------------------------------------------------------------------------
def normalize_model(counts, bits):
    """-> (cum[257] np.uint32, events): the scaled cumulative counts of a block with these 256 symbol counts, and one
    event (loser i, victim index, victim range before the steal) for every slot that normalize() moves."""
    counts = [int(c) for c in counts]
    assert len(counts) == 256 and sum(counts) > 0
    total, target = sum(counts), 1 << bits
    cum = [0] * 257
    for i in range(256):
        cum[i + 1] = cum[i] + counts[i]
    cum = [(target * c) // total for c in cum]                     # :142
    events = []
    for i in range(256):
        if counts[i] and cum[i + 1] == cum[i]:                     # :145
            best_freq, best = 1 << 32, -1
            for j in range(256):
                freq = cum[j + 1] - cum[j]
                if 1 < freq < best_freq:                           # the first smallest range above 1
                    best_freq, best = freq, j
            events.append((i, best, best_freq))
            if 0 <= best < i:                                      # :156
                for j in range(best + 1, i + 1):
                    cum[j] -= 1
            else:
                for j in range(i + 1, best + 1):
                    cum[j] += 1
    return np.array(cum, np.uint32), events


def emitted(data, simd):
    """-> per symbol (np.uint8, index = position in `data`) what the reference's encoder puts out in front of coding it:
    bytes (0 .. 2) for the one-state, 14-bit format, words (0 or 1) for the eight-state, 12-bit format."""
    data = np.ascontiguousarray(data, np.uint8)
    bits = BITS[bool(simd)]
    cum, _ = normalize_model(np.bincount(data, minlength=256), bits)
    start = [int(c) for c in cum[:256]]
    freq = [int(c) for c in np.diff(cum.astype(np.int64))]
    out = np.zeros(len(data), np.uint8)
    syms = data.tolist()
    if simd:
        states = [1 << 16] * 8                                     # cppans.h:585-588
        for i in range(len(syms) - 1, -1, -1):
            s = syms[i]
            x = states[i & 7]
            if ((freq[s] << 20) & 0xFFFFFFFF) <= x:                # :357; freq 4096: 2^32 wraps to 0, a word every symbol
                out[i] = 1
                x >>= 16
            states[i & 7] = ((x // freq[s]) << 12) + x % freq[s] + start[s]
    else:
        x = 1 << 23                                                # :260-263
        for i in range(len(syms) - 1, -1, -1):
            s = syms[i]
            x_max = freq[s] << 17                                  # :203
            k = 0
            while x_max <= x:                                      # :272-279
                x >>= 8
                k += 1
            out[i] = k
            x = ((x // freq[s]) << 14) + x % freq[s] + start[s]
    return out


def window_sums(per_symbol, width):
    """Sums over the windows [width * w, width * (w + 1)) from the block's start (the last one may be short)."""
    v = np.asarray(per_symbol, np.int64)
    pad = (-len(v)) % width
    return np.concatenate([v, np.zeros(pad, np.int64)]).reshape(-1, width).sum(axis=1)


# ---- blocks from counts ------------------------------------------------------------------------------------------------
def from_counts(counts, seed):
    """The block with these symbol counts, shuffled."""
    block = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(counts, np.int64))
    np.random.RandomState(seed).shuffle(block)
    return block


def _spread(lo, hi, k, avoid=()):
    """k indices spread evenly over [lo, hi), none of them in `avoid` (all there are, if those are fewer)."""
    pool = [i for i in range(lo, hi) if i not in avoid]
    k = min(k, len(pool))
    return [pool[(2 * t + 1) * len(pool) // (2 * k)] for t in range(k)]


def victim_counts(lane):
    """The counts of victim_cases()' block for lane range `lane`, and its two victims (first, second)."""
    a, b = 32 * lane + 31, (32 * lane + 32) % 256        # neighbours across a lane border (lane 7: 255 and 0)
    first, second = min(a, b), max(a, b)
    dominant = (32 * lane + 140) % 256
    small = 34 if lane % 2 else 51                         # scaled ranges 2 / 8 or 3 / 12 (12 / 14 bits)
    counts = np.zeros(256, np.int64)
    counts[a] = counts[b] = small
    taken = (a, b, dominant)
    if lane == 7:                                          # every other symbol lies between the victims
        losers = _spread(1, 255, 64, taken)
    else:
        losers = _spread(0, first, 2 + 3 * lane, taken) + _spread(second + 1, 256, 40, taken)
    counts[losers] = 1
    counts[dominant] = LOSER_BLOCK - int(counts.sum())
    return counts, first, second


def tie_counts(lane):
    """The counts of victim_cases()' "tie" block for lane range `lane`, and its two victims (first, second)."""
    a, b = 32 * lane + 31, (32 * lane + 32) % 256
    first, second = min(a, b), max(a, b)
    below, above, dominant = (60, 190, 128) if lane == 7 else (first - 3, second + 2, second + 5)
    counts = np.zeros(256, np.int64)
    counts[a] = counts[b] = 51
    counts[below] = counts[above] = 1
    counts[dominant] = LOSER_BLOCK - int(counts.sum())
    return counts, first, second


def victim_cases():
    """name -> block, all of LOSER_BLOCK = 4096 x 17 bytes, so that a count of c takes exactly c / 17 slots of the 12-bit
    table and 4 c / 17 of the 14-bit one wherever it lies, when c is a multiple of 17, and a symbol that occurs once is
    left without a slot at 16 of 17 places (12 bits) or 13 of 17 (14 bits): a loser.

    "lane L", L = 0 .. 7: a dominant symbol; two victims of the same count (51: ranges 3 and 12; for odd L 34: ranges 2
    and 8) at 32 L + 31 and at the first index of the next lane's range (L = 7: at 255 and at 0), so the first steal
    meets a tie between two lanes of the octet that must go to the lower index; losers below the victims (2 + 3 L of
    them; for L = 7 all lie between the two) and 40 above (L = 6: the 31 there are).  Each steal wears the victim down
    by one; at a range of 1 it is no victim any more and the steals move to the other one, then to the dominant symbol.
    "tie L": the same two victims (count 51) and the dominant symbol, but only two losers, one on either side: fewer
    steals than wear one victim out, so the table that results says which of the two the tie went to.  (In a "lane L"
    block both victims end at a range of 1 whichever went first.)
    "dominant 0" / "dominant 255": the dominant symbol at an end of the table, 60 losers all above / all below it."""
    out = {}
    for lane in range(8):
        counts, _, _ = victim_counts(lane)
        out[f"lane {lane}"] = from_counts(counts, 100 + lane)
    for lane in range(8):
        out[f"tie {lane}"] = from_counts(tie_counts(lane)[0], 150 + lane)
    for name, dominant, losers in (("dominant 0", 0, _spread(1, 256, 60)), ("dominant 255", 255, _spread(0, 255, 60))):
        counts = np.zeros(256, np.int64)
        counts[losers] = 1
        counts[dominant] = LOSER_BLOCK - 60
        out[name] = from_counts(counts, 200 + dominant)
    return out


def singletons():
    """255 symbols once each and symbol 128 seventy thousand times: as many steals as a block can ask for, all from one
    victim in the middle of the table, in both directions."""
    counts = np.ones(256, np.int64)
    counts[128] = 70000
    return from_counts(counts, 300)


DENSE_RARE_HEADS = (0, 1, 7, 8, 15, 16)


def dense_rare(head):
    """head + 40000 zeros, a seeded permutation of 1 .. 255, 30000 zeros.  The 255 symbols in a row have a range of 1
    each: the one-state encoder puts out up to two bytes for each, the eight-state encoder a word -- as fast as either
    format can -- and `head` moves the run through the phases of the 8-symbol rounds and 16-symbol chunks."""
    run = (np.random.RandomState(400).permutation(255) + 1).astype(np.uint8)
    return np.concatenate([np.zeros(head + 40000, np.uint8), run, np.zeros(30000, np.uint8)])


ONE_SYMBOL_LENGTHS = (1, 7, 8, 9, 64, 65, 4096, 70000)


def one_symbol(n):
    """n times the byte 0xA5: its frequency is the whole table, 4096 (x_max wraps to 0: a word for every symbol) or
    16384 (x_max = 2^31: no byte ever leaves)."""
    return np.full(n, 0xA5, np.uint8)


ALL_256_REPS = (1, 3)


def all_256(reps):
    """All 256 symbols `reps` times each, shuffled: every entry of the eight-state decoder's first[] / table[] window."""
    return from_counts(np.full(256, reps, np.int64), 500 + reps)


def rare_item(n, seed):
    """An item in the manner of dense_rare: n bytes, zeros around a run of min(255, n / 2) different other bytes."""
    m = min(255, n // 2)
    run = (np.random.RandomState(seed).permutation(255)[:m] + 1).astype(np.uint8)
    at = (n - m) // 2
    return np.concatenate([np.zeros(at, np.uint8), run, np.zeros(n - m - at, np.uint8)])


def block_cases():
    """name -> block: every block builder above at every parameter it is meant for."""
    out = {f"victims, {k}": v for k, v in victim_cases().items()}
    out["singletons"] = singletons()
    out.update({f"dense_rare({h})": dense_rare(h) for h in DENSE_RARE_HEADS})
    out.update({f"one_symbol({n})": one_symbol(n) for n in ONE_SYMBOL_LENGTHS})
    out.update({f"all_256({r})": all_256(r) for r in ALL_256_REPS})
    return out


PADDED_BLOCK = 131072


def padded_order(count):
    """Block b of a padded call is case padded_order(count)[b]."""
    order = [(9 * k) % count for k in range(count)]
    assert sorted(order) == list(range(count))
    return order


def padded_call(cases, filler, block=PADDED_BLOCK, seed=600):
    """The blocks of `cases` in one buffer, each filled up to `block` bytes: with seeded random bytes of its own
    ("seeded": every symbol then occurs some hundred times, the case only tilts the model and nothing is stolen), or with
    the case's own most frequent byte ("dominant": the symbols that occur once still do, so eight blocks of a wave run
    steal loops of different lengths, with different victims, side by side).  The cases are dealt out in steps of nine,
    so that every wave gets some of each builder (padded_order)."""
    assert filler in ("seeded", "dominant")
    rs = np.random.RandomState(seed)
    parts = []
    names = list(cases)
    for k in padded_order(len(names)):
        v = cases[names[k]]
        assert len(v) <= block
        fill = rs.randint(0, 256, block - len(v)).astype(np.uint8)
        if filler == "dominant":
            fill[:] = np.argmax(np.bincount(v, minlength=256))
        parts += [v, fill]
    return np.concatenate(parts)


# ---- item lengths: blocks of chosen lengths side by side in a wave (csrc/rcx_items.hpp) --------------------------------------
def item_class_upper(length):
    """rcx_items.hpp item_class_upper(): the power of two at or above the length, 16 at the least.  The item encoders get
    one launch per class, in work order (longest first); the decoders one launch for all entries."""
    up = 16
    while up < length:
        up <<= 1
    return up


# One class, (512, 1024]: the eight items are one wave of the eight-state encoder, and of its decoder.  Every length but
# the last is a multiple of 8, so from an 8-aligned buffer every item starts 8-aligned: by_eights and out8 hold; the
# rounds behind each block's last one are 127 ... 64, so `common` is 64 below a longest of 128; groups & ~7 are 128 ... 64,
# so fast_groups is 64.
WAVE_SAME_CLASS = [1024, 1000, 776, 640, 584, 576, 520, 515]
# Three bytes more each: at whatever offset the buffer starts, seven of the eight items or all of them are off an 8-byte
# border, so by_eights fails, fast_groups is 0 and the slow loops carry everything.  (1027 is a class of its own.)
WAVE_SAME_CLASS_PLUS_3 = [n + 3 for n in WAVE_SAME_CLASS]
# Lengths from 4096 down to 1, tails (len & 7) of 0, 1, 5 and 7, groups & 7 zero and not.  The decoders take the whole
# work order in one launch: the eight-state decoder seats it in two waves, 4096 ... 17 and 16 ... 1; the one-state decoder
# in one wave when it runs 16 blocks a wave, in four when it runs 4 (quad_waves; by default, with so few entries, it runs
# one block a wave).  The encoders see seven classes of one or two items and one of five: live octets among idle ones
# in every wave.
WAVE_MIXED = [4096, 1029, 520, 129, 72, 64, 63, 17, 16, 9, 8, 7, 1]
# 64 lengths of one class, (256, 512], every residue modulo 16 four times: one workgroup of rcx_enc_rans1w_k, whose
# nchunks = 32 follows the longest block while the others end 0 ... 11 chunks earlier, each at its own place in a chunk.
RANS1_WORKGROUP = [512 - 3 * k for k in range(64)]

LENGTH_SETS = {"same class": WAVE_SAME_CLASS, "same class + 3": WAVE_SAME_CLASS_PLUS_3, "mixed": WAVE_MIXED,
               "rans1 workgroup": RANS1_WORKGROUP}


def quad_waves(lengths, quads):
    """The lengths that share a wave of the one-state decoder (rcx_dec_rans1_quad_k) at `quads` blocks a wave: the work
    order cut into runs of `quads` (rcx_quad.hpp RCX_QUAD_SEAT: block = (workgroup x waves + wave) x quads + quad)."""
    ordered = [lengths[k] for k in work_order(lengths)]
    return [ordered[w: w + quads] for w in range(0, len(ordered), quads)]


def work_order(lengths):
    """Indices in the order the item calls work in: by length, longest first, then the caller's order."""
    return sorted(range(len(lengths)), key=lambda k: (-lengths[k], k))
