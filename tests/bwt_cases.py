"""Inputs for the block-sort (blksort.h) parity tests, built from integer arithmetic only so that the same bytes come
out on every machine and numpy version.  tests/golden/make_golden_bwt.py runs the REAL reference over them and stores
what it produced (tests/golden/bwt.json); the tests run the oracle and the GPU path over the same inputs.

A case is a name -> bytes.  The block size is fixed by the reference (32768, blksort.h:82); what exercises the code is
the content: ordinary data, long repeats (deep comparisons), and periodic blocks, where the rotations tie and the row
index the reference stores depends on the moves of its unstable sort (oracle/bwt_oracle.c).
"""
from __future__ import annotations

import numpy as np

BLOCK = 32768
ENCODED = BLOCK + 2


def mix(n: int, seed: int) -> np.ndarray:
    """n pseudo-random bytes: splitmix64 of (seed, index), top byte."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    return (x >> np.uint64(56)).astype(np.uint8)


def _tile(word: np.ndarray, n: int = BLOCK) -> np.ndarray:
    return np.resize(word, n).astype(np.uint8)


def periodic(p: int, seed: int, alphabet: int = 256) -> np.ndarray:
    """A block of period p.  The word is random, so p is its primitive period with near certainty; seeds below were
    chosen (and are checked in the generator) so that it is."""
    return _tile((mix(p, seed).astype(np.uint32) % alphabet).astype(np.uint8))


def cases() -> dict[str, np.ndarray]:
    c: dict[str, np.ndarray] = {}
    c["random 2 blocks + tail"] = mix(2 * BLOCK + 1234, 1)
    c["tail only"] = mix(1000, 2)
    c["empty"] = np.zeros(0, np.uint8)
    c["four letters"] = (mix(BLOCK, 3) % 4 + 97).astype(np.uint8)
    c["two letters"] = (mix(BLOCK, 4) % 2 + 97).astype(np.uint8)
    c["runs of 64"] = np.repeat(mix(BLOCK // 64, 5), 64)
    c["repeat of 5000"] = _tile(mix(5000, 6))            # long common prefixes, not periodic in 32768
    c["repeat of 12288 + 1"] = np.concatenate([_tile(mix(12288, 7))[:-1], np.array([0x5A], np.uint8)])
    c["zeros"] = np.zeros(BLOCK, np.uint8)               # every rotation ties
    c["ones then a two"] = np.concatenate([np.ones(BLOCK - 1, np.uint8), np.array([2], np.uint8)])  # almost periodic
    c["ab..ab then aa"] = np.concatenate([_tile(np.frombuffer(b"ab", np.uint8))[:-2], np.frombuffer(b"aa", np.uint8)])
    for p, seed, alphabet in ((2, 11, 256), (4, 12, 256), (4, 13, 3), (16, 14, 256), (64, 15, 3), (256, 16, 256),
                              (1024, 17, 4), (4096, 18, 256), (16384, 19, 256), (16384, 20, 2)):
        c[f"period {p} (seed {seed}, {alphabet} symbols)"] = periodic(p, seed, alphabet)
    # unbalanced partitions: the reference's sort runs out of its 11 levels and falls back to heapsort (blksort.h:284-287)
    c["period 8192, skewed bytes"] = _tile(np.minimum(mix(8192, 100), 40).astype(np.uint8))
    c["period 4096, ramp"] = _tile((np.arange(4096) // 16).astype(np.uint8))
    c["period 2048, sorted"] = _tile(np.sort(mix(2048, 6)))
    # a period that is one long run and a single other byte: every partition pass of the reference's sort peels off two
    # rows, so its replay makes thousands of passes over thousands of rows (the replay's worst case, csrc/rcx_bwt_tie.hpp)
    c["period 16384, a run then b"] = _tile(np.concatenate([np.full(16383, 97, np.uint8), np.array([98], np.uint8)]))
    c["period 4096, a run then b"] = _tile(np.concatenate([np.full(4095, 97, np.uint8), np.array([98], np.uint8)]))
    c["period 8192, b then a run"] = _tile(np.concatenate([np.array([98], np.uint8), np.full(8191, 97, np.uint8)]))
    c["skewed bytes"] = np.minimum(mix(BLOCK, 101), 24).astype(np.uint8)   # not periodic, heapsort all the same
    # long runs of one byte (1 .. 4096 long): on the GPU such blocks start from run keys, not from two bytes
    c["long runs, two blocks"] = np.repeat(mix(64, 23), 1 + (mix(64, 24).astype(np.uint32) * 16 + mix(64, 25) % 16))[: 2 * BLOCK]
    c["three blocks: periodic, random, zeros"] = np.concatenate([periodic(8, 21), mix(BLOCK, 22), np.zeros(BLOCK + 77, np.uint8)])
    return c


# the subset the CPU suite runs the (slow on ties: ~1.5 s a block, like the reference) oracle over
CPU_SUBSET = ("random 2 blocks + tail", "tail only", "empty", "four letters", "runs of 64", "repeat of 5000", "zeros",
              "ones then a two", "period 2 (seed 11, 256 symbols)", "period 4 (seed 13, 3 symbols)",
              "period 256 (seed 16, 256 symbols)", "period 16384 (seed 20, 2 symbols)")


# ---- blocks at the forward kernel's switch points (csrc/rcx_bwt.hpp, rcx_bwt_fwd_k) ---------------------------------------
LIST_LENGTHS = (1024, 3072, 11264)   # entries of the three list forms: 1024 x (1, RCX_BWT_LIST_SMALL, RCX_BWT_LIST_BIG)
RUNNY = BLOCK // 8                   # RCX_BWT_RUNNY: fewer changes than this and the block starts from run keys
LADDER_DEPTH = 8                     # the ladders put their counts into the round with this shift
ROTATIONS = (1, 31, 32, 16385)       # places a run-keyed block is turned by, so that a run straddles its end


def changes(block: np.ndarray) -> int:
    """The number of places, cyclically, where a byte differs from the next: what the kernel holds against RUNNY."""
    return int(np.count_nonzero(block != np.roll(block, -1)))


def open_counts(block: np.ndarray) -> dict[int, int]:
    """d -> the number of rotations whose first d bytes, cyclically, are shared with another rotation, d = 2, 4, 8, ...
    up to the first depth at which there is none (or the block's length).  Prefix doubling on integers: the class of a
    rotation's first 2d bytes is the pair of the classes of its two halves.

    This is a MODEL of the kernel's `open`, read from its code, not a measurement -- the kernel cannot report the
    count.  By rcx_bwt_rerank (`left`) and rcx_bwt_place (its return value) the round with shift h of a block that
    starts from two-byte keys (changes(block) >= RUNNY) begins with open == open_counts(block)[h]; h = 2 is the state
    behind the two-byte start.  Tests that aim at a value of `open` therefore use ladders of neighbouring values."""
    n = len(block)
    cls = block.astype(np.int64)
    out, d = {}, 1
    while d < n:
        pair = cls * n + np.roll(cls, -d)
        _, cls, count = np.unique(pair, return_inverse=True, return_counts=True)
        cls = cls.reshape(-1).astype(np.int64)
        d *= 2
        out[d] = int(np.count_nonzero(count[cls] > 1))
        if out[d] == 0:
            break
    return out


def planted(seed: int, twice: int, thrice: int = 0) -> np.ndarray:
    """mix(BLOCK, seed) with one stretch of `twice` bytes in two places and, if asked for, another of `thrice` bytes in
    three.  A stretch of L bytes in k places leaves k (L - d + 1) rotations open at depth d (while d <= L, and as long
    as the bytes around the copies differ, which open_counts shows); a pair and a triple together give either parity."""
    b = mix(BLOCK, seed).copy()
    at = 0
    for length, copies in ((twice, 2), (thrice, 3)):
        if length:
            for c in range(1, copies):
                b[at + c * (length + 1): at + c * (length + 1) + length] = b[at: at + length]
            at += copies * (length + 1) + 1
    assert at <= BLOCK
    return b


def open_ladder(limit: int, reach: int = 3, seed: int = 40) -> list[np.ndarray]:
    """2 reach + 1 blocks whose open_counts at LADDER_DEPTH are limit - reach ... limit + reach, in that order."""
    blocks = []
    for v in range(limit - reach, limit + reach + 1):
        if v % 2 == 0:
            blocks.append(planted(seed, v // 2 + LADDER_DEPTH - 1))
        else:  # 3 a + 2 b = v with a odd: b is 1, 2 or 3
            a = (v - 2) // 3
            a -= 1 - a % 2
            blocks.append(planted(seed, (v - 3 * a) // 2 + LADDER_DEPTH - 1, a + LADDER_DEPTH - 1))
    return blocks


def runs_block(nruns: int, seed: int) -> np.ndarray:
    """A block of `nruns` runs (BLOCK / 16 < nruns < BLOCK / 2) whose neighbouring bytes differ, the last run's and the
    first's included: changes() == nruns.  Lengths: BLOCK spread evenly over the runs, then every second run gives some
    of its bytes to the one before it, so the lengths differ (1 byte at the least) and still sum to BLOCK."""
    q, r = divmod(BLOCK, nruns)
    lens = np.full(nruns, q, np.int64)
    lens[:r] += 1
    give = mix(nruns // 2, seed).astype(np.int64) % q
    lens[0: 2 * (nruns // 2): 2] += give
    lens[1::2] -= give
    vals = np.cumsum(1 + mix(nruns, seed + 1).astype(np.int64) % 200) % 256   # steps of 1 .. 200: never the byte before
    if vals[-1] == vals[0]:
        vals[-1] = next(v for v in range(256) if v not in (vals[0], vals[-2]))
    return np.repeat(vals.astype(np.uint8), lens)


def runny_ladder() -> list[np.ndarray]:
    """Nine blocks with changes() = RUNNY - 4 ... RUNNY + 4: the first four start from run keys, the others from two
    bytes.  Every other one is turned by three places, so that a run straddles the block's end."""
    out = []
    for i, c in enumerate(range(RUNNY - 4, RUNNY + 5)):
        b = runs_block(c, 500 + i)
        out.append(np.roll(b, 3) if i % 2 else b)
    return out


def _runs(pairs) -> np.ndarray:
    return np.concatenate([np.full(n, v, np.uint8) for v, n in pairs])


def aligned_runs() -> np.ndarray:
    """Runs of 31, 32, 33, 63, 64 and 65 bytes, each starting at places 0, 1 and 31 modulo 32 (a filler run in front of
    each brings it there); bytes cycle through 1 .. 250 so that neighbours differ; one long run of zeros fills the block."""
    pairs, at, v = [], 0, 0
    for start in (0, 1, 31):
        for length in (31, 32, 33, 63, 64, 65):
            fill = (start - at) % 32 or 32
            for n in (fill, length):
                pairs.append((1 + v % 250, n))
                v += 1
                at += n
    pairs.append((0, BLOCK - at))
    return _runs(pairs)


def tied_runs() -> np.ndarray:
    """700 times 20 a's and 20 b's: 699 runs of a and 699 of b share byte, length and the byte behind them, so their run
    keys tie and the rounds tell them apart; runs of 16 .. 31 bytes of other values fill the block."""
    pairs = [(97, 20), (98, 20)] * 700
    at, i = 28000, 0
    vals, lens = mix(400, 61), mix(400, 62)
    while at < BLOCK:
        n = min(16 + int(lens[i]) % 16, BLOCK - at)
        pairs.append((100 + (int(vals[i]) % 64) * 2 + i % 2, n))   # (parity alternates: never the byte before)
        at += n
        i += 1
    return _runs(pairs)


def run_key_cases() -> dict[str, np.ndarray]:
    """Blocks that start from run keys (changes() < RUNNY), each as built and turned right by ROTATIONS places, where
    its first and last byte are one run that wraps round the block's end."""
    c = cases()
    a, b = np.uint8(97), np.uint8(98)
    base = {"two runs of 16384": _runs([(a, 16384), (b, 16384)])}
    for k in (1, 31, 32, 33):
        base[f"a^{k} then b"] = _runs([(a, k), (b, BLOCK - k)])
    base["ones, a two in the middle"] = np.roll(c["ones then a two"], 16385)   # the two at place 16384
    base["aligned runs"] = aligned_runs()
    base["tied runs"] = tied_runs()
    base["runs of 64"] = c["runs of 64"]
    for i in range(2):
        base[f"long runs, block {i}"] = c["long runs, two blocks"][i * BLOCK: (i + 1) * BLOCK]
    out = {}
    for name, block in base.items():
        out[name] = block
        for r in ROTATIONS:
            out[f"{name}, turned by {r}"] = np.roll(block, r)
    return out


def rows(enc: np.ndarray) -> list[int]:
    """The row index stored behind every whole block of an encoded buffer."""
    nb = len(enc) // ENCODED
    return [int(enc[b * ENCODED + BLOCK]) | int(enc[b * ENCODED + BLOCK + 1]) << 8 for b in range(nb)]


def primitive_period(block: np.ndarray) -> int:
    n = len(block)
    p = 1
    while p < n:
        if n % p == 0 and np.array_equal(block, np.roll(block, -p)):
            return p
        p *= 2
    return n
