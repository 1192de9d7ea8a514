"""The adaptive coder's interval walked in exact integers, and streams made from it whose target lies past the table.

A target past the table cannot be had by flipping payload bytes at random: low stays below range on any input, and only
the last (range mod total) values below range are past the table.  So the stream is made: the coder's interval along the
block's first i symbols is walked in exact integers (range depends on the symbols alone; the decoder's low is the stream's
bytes so far, as one big-endian number, minus the interval's lower end), and the bytes the decoder has consumed when it
looks for symbol i are set to the number that puts low into those last values.
Shared by the decoder tests that need such streams (tests written before this module carry a copy of their own).
"""
import numpy as np


def walk(symbols, steps):
    """The decoder's state in front of symbol i, for i = 0 .. steps: (i, lower end, range, t, total, bytes consumed
    counted from byte 4 of the stream).  include/rcx.h: every count starts at 1; range starts at 2^24 - 1 behind the
    four bytes of low; range is shifted up by whole bytes until its top byte is not 0, then t = range / total."""
    counts = np.ones(256, np.int64)
    total, rng, lower, nbytes = 256, 0x00FFFFFF, 0, 4
    for i in range(steps + 1):
        k = (32 - rng.bit_length()) // 8
        rng <<= 8 * k
        lower <<= 8 * k
        nbytes += k
        t = rng // total
        yield i, lower, rng, t, total, nbytes
        s = int(symbols[i])
        lower += int(counts[:s].sum()) * t
        rng = int(counts[s]) * t
        counts[s] += 1
        total += 1


def past_the_table(d, b, position, groups=range(20, 40)):
    """Block b's stream (d: gpu_support.Damaged) with the target of one symbol at in-group position `position` past the
    table, then runs of 0xFF and of 0x00, then random bytes -> (stream, symbol index); None if none of `groups` leaves room behind the table there.
    From the 20th group on the quad decoder's scratch row, which it then reads as counts, already holds parked output."""
    good, orig = d.good(b), d.orig[b]
    want = {16 * g + position for g in groups}
    for i, lower, rng, t, total, nbytes in walk(good, max(want)):
        low = int.from_bytes(orig[4: 4 + nbytes].tobytes(), "big") - lower
        below = int(np.count_nonzero(good[:i] < good[i])) + int(good[i])  # cumulative count under symbol i
        mine = int(np.count_nonzero(good[:i] == good[i])) + 1
        assert below * t <= low < (below + mine) * t, (i, "the walk left the reference's interval")
        room = rng - total * t
        if i in want and room > 0:
            s = d.padded(b)
            code = lower + total * t + room // 2
            s[4: 4 + nbytes] = np.frombuffer(code.to_bytes(nbytes, "big"), np.uint8)
            at = 4 + nbytes
            for r, fill in enumerate((0xFF, 0x00, 0xFF, 0x00)):
                s[at + 48 * r: at + 48 * (r + 1)] = fill
            return s, i
    return None
