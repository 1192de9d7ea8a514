"""Damaged streams (include/rcx.h, "Damaged streams"): oracle streams with some blocks damaged on purpose, and the recipe
that places damage of every kind a coder has where the kernels' paths part.  Pure: numpy, the oracle and the constants of
cpprcoder_amd.rcx, no GPU and no torch, so that tests/crafted_cases.py can list these streams for the comparison with the
reference build.  The GPU tests take all of this through tests/gpu_support.py, which hands it on.
"""
import numpy as np

from cpprcoder_amd import rcx, workloads

HEAD = {0: 5, 1: 516, 2: 1032, 3: 1032}  # bytes in front of the coded payload: header (+ the adaptive coder's 0x00 / table)
LOW = {0: (5, 9), 1: (516, 521)}          # the bytes the first renormalisation shifts in (the static coder skips 516)
# per coder; the static coder's bytes use every value, so no count is 0 and its damaged streams decode (see Damaged.damage)
DATA = ("zipf", "uniform", "zipf", "canterbury")
COUNT0 = "past the table onto a count of 0"


def oracle_decode_one(oracle, stream, length, coder, block):
    """The oracle on one stream alone, reading no byte past it -> (every symbol decoded, bytes).  `block` is the block
    size the oracle is told (it sizes its sink from it); each caller passes its own."""
    slots = np.zeros((1, len(stream) + 64), np.uint8)
    slots[0, : len(stream)] = stream
    out, ok = oracle.decode_blocks(slots, np.array([len(stream)], np.uint32), block, length, coder=coder)
    return ok, out


def first_wrong(oracle, stream, good, block, coder):
    ok, out = oracle_decode_one(oracle, stream, len(good), coder, block)
    if not ok:
        return None
    diff = np.nonzero(out != good)[0]
    return int(diff[0]) if len(diff) else None


def flip_at_symbol(oracle, stream, size, good, block, coder, targets):
    """A single byte flip in `stream` (`size` bytes of stream, then padding) whose first wrong symbol is one of `targets`
    (a set of symbol indices), found by trying positions around the one that an even spread of the bytes gives."""
    lo = HEAD[coder] + 4
    pay = size - lo
    for want in sorted(targets):
        guess = lo + int(pay * want / max(len(good), 1))
        for p in sorted(range(max(lo, guess - 48), min(len(stream) - 4, guess + 48)), key=lambda q: abs(q - guess)):
            for x in (0x01, 0x80, 0x5A):
                s = stream.copy()
                s[p] ^= x
                if first_wrong(oracle, s, good, block, coder) in targets:
                    return s
    return None


class Damaged:
    """Oracle streams of `data` with some blocks damaged: slots (rows padded as needed), sizes, and per block the kind."""

    def __init__(self, oracle, data, block, coder, seed):
        self.oracle, self.data, self.block, self.coder = oracle, data, block, coder
        self.rs = np.random.RandomState(seed)
        slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=8)
        self.nblocks = len(sizes)
        self.pad = 3 * block
        self.orig = [slots[b, : int(sizes[b])].copy() for b in range(self.nblocks)]
        self.rows = list(self.orig)
        self.kind = {}

    def length(self, b):
        return min(self.block, len(self.data) - b * self.block)

    def good(self, b):
        return self.data[b * self.block: b * self.block + self.length(b)]

    def padded(self, b):
        return np.concatenate([self.orig[b], self.rs.randint(0, 256, self.pad).astype(np.uint8)])

    def decode_one(self, b):
        """The oracle on block b's stream as it is now, alone -> (ok, bytes)."""
        return oracle_decode_one(self.oracle, self.rows[b], self.length(b), self.coder, self.block)

    def damage(self, b, kind, stream, fails=False):
        """fails: the reference cannot decode this stream, padding or not.  That is only the static coder's symbol of count
        0: find() (cpprcoder.h:521-535) never fails -- a target at or past the total falls through to symbol 255 -- but if
        the symbol it gives has count 0, range becomes 0 and the renormalisation (:506-513) runs dry.  Every other damaged
        stream here is padded so that the oracle decodes it completely, and that is checked."""
        ok, _ = oracle_decode_one(self.oracle, stream, self.length(b), self.coder, self.block)
        assert ok != fails, f"block {b} ({kind}): the oracle {'decodes' if ok else 'fails on'} it"
        self.rows[b], self.kind[b] = stream, kind

    def restore(self, b):
        self.rows[b] = self.orig[b]
        self.kind.pop(b, None)

    def truncate(self, b, k):
        self.rows[b], self.kind[b] = self.orig[b][:-k], f"truncated by {k}"

    def streams(self):
        sizes = np.array([len(r) for r in self.rows], np.uint64)
        offsets = np.zeros(self.nblocks + 1, np.uint64)
        np.cumsum(sizes, out=offsets[1:])
        return np.concatenate(self.rows), offsets

    def expected(self):
        """-> (status, first bad block or None, {block: expected bytes} for the blocks whose bytes are asserted)"""
        bad, want = [], {}
        for b in range(self.nblocks):
            if b not in self.kind:
                want[b] = self.good(b)
                continue
            ok, out = self.decode_one(b)
            if not ok:
                bad.append(b)
            else:  # (a truncated stream the reference still decodes completely included)
                want[b] = out
        return (rcx.E_CORRUPT if bad else rcx.OK), (bad[0] if bad else None), want


def build(oracle, coder, block, nblocks, seed):
    """About nblocks blocks, the last one ragged; damage of every kind the coder has, in blocks spread over the call."""
    data = workloads.by_name(DATA[coder], (nblocks - 1) * block + block // 4 + 7, seed)
    d = Damaged(oracle, data, block, coder, seed)
    groups = block // 16
    b = 1
    if coder in LOW:
        s = d.padded(b)
        s[LOW[coder][0]: LOW[coder][1]] = 0xFF  # the first target at or past the table
        d.damage(b, "first target past the table", s)
        b += 2
        for name, targets in (("group position 0", {16 * g for g in range(3, 12)}), ("group position 1", {16 * g + 1 for g in range(3, 12)}),
                              ("group position 15", {16 * g + 15 for g in range(3, 12)}),
                              ("last group of the fast loop", set(range(16 * (groups - 1), 16 * groups - 2)))):
            s = flip_at_symbol(oracle, d.padded(b), len(d.orig[b]), d.good(b), block, coder, targets)
            assert s is not None, name
            d.damage(b, name, s)
            b += 2
        for name, fill in (("run of 0xFF", 0xFF), ("run of 0x00", 0x00)):
            s = d.padded(b)
            at = HEAD[coder] + 4 + (len(d.orig[b]) - HEAD[coder]) // 2
            s[at: at + 48] = fill
            d.damage(b, name, s)
            b += 2
    if coder == rcx.CODER_STATIC:
        for name in ("count to 0", "count moved"):
            s = d.padded(b)
            counts = s[4:516].view("<u2").copy()
            used = np.nonzero(counts)[0]
            src, dst = used[len(used) // 2], used[0]
            if name == "count moved":
                counts[dst] = min(int(counts[dst]) + int(counts[src]), 0xFFFF)
            counts[src] = 0
            s[4:516] = counts.view(np.uint8)
            d.damage(b, name, s)
            b += 2
        # the first target past the table, where find() falls through to symbol 255, whose count is now 0: range 0, the
        # reference runs dry whatever follows (cpprcoder.h:500-513), so the call reports RCX_E_CORRUPT for this block
        s = d.padded(b)
        s[4 + 2 * 255: 4 + 2 * 256] = 0
        s[LOW[coder][0]: LOW[coder][1]] = 0xFF
        d.damage(b, COUNT0, s, fails=True)
        b += 2
    if coder in (rcx.CODER_RANS, rcx.CODER_RANS8):
        for i in range(4):
            s = d.padded(b)
            z = len(d.orig[b])
            for _ in range(1 + i):
                s[int(d.rs.randint(HEAD[coder] + 16, z))] ^= int(d.rs.randint(1, 256))
            d.damage(b, f"payload flips ({1 + i})", s)
            b += 2
    last = d.nblocks - 1  # the ragged last block: a flip in its symbol-by-symbol tail
    if coder in LOW:
        n_last = d.length(last)
        s = flip_at_symbol(oracle, d.padded(last), len(d.orig[last]), d.good(last), block, coder, set(range(16 * (n_last // 16), n_last)))
        assert s is not None, "tail flip"
        d.damage(last, "flip in the tail", s)
    return d
