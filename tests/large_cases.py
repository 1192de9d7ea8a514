"""What the tests past 4 GiB share (tests/test_large_cases_cpu.py, tests/test_gpu_past_4gib.py): a buffer that is periodic, so
that nothing of its size is ever made or compared on the CPU.  Not a test file.

A TILE of T = 8 MiB (128 blocks of 64 KiB, 256 block-sort blocks, 16 superblocks of width 8) is repeated K = 513 times on the
device, and TAIL = 12345 bytes of the tile follow: N = 513 * 2^23 + 12345 = 4 303 368 249 bytes.  Period 256 begins at 2^31,
period 512 begins at exactly 2^32 and lies wholly past it, the last block is short, and TAIL is odd: every width has tail
bytes.  Every operation of the library is independent per block, superblock or item, so the result of period j >= 1 must
equal that of period 0 -- compared on the device (periodic_equal, periodic_table) -- and only period 0 and the tail are
compared with the CPU oracle or a numpy restatement, whose input is the tile alone.

What this cannot see: a defect that is itself periodic in 8 MiB.  Period 512 begins exactly at 2^32 and the tail is ragged,
so a WRITE position that wrapped at 2^32 leaves period 512's own place unwritten (the destinations are filled with a guard
byte) and lands in a payload whose periods are no divisor of 2^32.  But a SOURCE position that wrapped there would read period
0's bytes, which are equal, and the tail's from period 1: on_device(..., last=other tile) puts another tile's bytes into
period 512 and the tail for the tests that look for exactly that.

The condition the block-coder tests rest on, stated here and checked with the oracle alone (test_large_cases_cpu.py):
    oracle sizes of the tile * 513 + the tail's stream > 2^32       for all four coders
so that the compacted payload passes 2^32 as well.  A uniform 64 KiB block costs the adaptive coder about 65 655 bytes; 128
of them are 8 403 840, and 513 periods pass 2^32 only while a period keeps more than 8 372 232 of them: the special
content of the coder tile may save no more than about 31 KiB a period.  So the special blocks are uniform blocks that BEGIN
with a special stretch of SPECIAL bytes (all 0x00, all 0xFF, two kinds of runs), not whole blocks of it.
"""
import functools

import numpy as np

from cpprcoder_amd import workloads

BLOCK = 65536
T = 8 << 20
K = 513
TAIL = 12345
N = K * T + TAIL
BLOCKS_PER_TILE = T // BLOCK                   # 128
NBLOCKS = K * BLOCKS_PER_TILE + 1              # the last one holds TAIL bytes
SPECIAL = 4096                                 # bytes of special content at the head of each special block
SPECIAL_BLOCKS = (1, 37, 64, 127)              # all 0x00, runs, all 0xFF, runs: the second block, two inside, the period's last
CODERS = (0, 1, 2, 3)

# the item pattern: lengths that sum to the tile
ITEM_SPECIAL = (0, 1, 16, 17, 4097, 65536, 65537, 200_000)


# ---- tiles -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile(kind):
    """The tile by content kind (read-only):
    coder   workloads.uniform bytes; four blocks begin with a special stretch (see the module's text)
    filter  random bytes; the second half holds the `minus_k` elements of predict_cases for widths 2, 4 and 8 in turn, a
            superblock of width 8 (512 KiB) each: every difference all 0xFF, the carry through every byte"""
    if kind == "coder":
        x = workloads.uniform(T, 4242)
        for b, fill in zip(SPECIAL_BLOCKS, ("zero", "runs", "ff", "runs")):
            at = b * BLOCK
            if fill == "runs":
                x[at: at + SPECIAL] = workloads.runs(SPECIAL, seed=b)
            else:
                x[at: at + SPECIAL] = 0 if fill == "zero" else 0xFF
    else:
        assert kind == "filter"
        import predict_cases
        x = workloads.uniform(T, 777)
        sb = 8 * BLOCK
        for s in range(8, 16):
            x[s * sb: (s + 1) * sb] = predict_cases.kernel_data("minus_k", (2, 4, 8)[s % 3], sb, None)
    x.setflags(write=False)
    return x


def tail_of(x):
    return x[:TAIL]


def on_device(x, offset=0, guard=64, fill=0xA5, last=None):
    """The periodic buffer of tile `x` on the device -> (whole, view): `view` is the N bytes, `offset` + guard bytes of `fill`
    in front of it and `guard` bytes behind it in `whole`.  With `last`, another tile, period K - 1 and the tail hold that
    tile's bytes: everything from 2^32 on differs from what lies 2^32 bytes in front of it, so that a SOURCE position which
    wrapped there reads other bytes (in the periodic buffer it would read equal ones and nothing would show)."""
    import torch
    whole, view = guarded(N, offset, guard, fill)
    t = torch.from_numpy(np.array(x, dtype=np.uint8)).cuda()  # (a copy: the tiles are read-only)
    view[: K * T].view(K, T).copy_(t.unsqueeze(0).expand(K, T))
    if last is not None:
        t = torch.from_numpy(np.array(last, dtype=np.uint8)).cuda()
        view[(K - 1) * T: K * T].copy_(t)
    view[K * T:].copy_(t[:TAIL])
    return whole, view


def guarded(nbytes, offset=0, guard=64, fill=0xA5):
    """-> (whole, view): nbytes at byte `offset` + guard of an allocation, everything set to `fill`."""
    import torch
    whole = torch.full((guard + offset + nbytes + guard,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[guard + offset: guard + offset + nbytes]


def all_bytes(t, value, step=1 << 30):
    """Every byte of t equals value (piece by piece: no temporary of t's size)."""
    return all(bool((t[at: at + step] == value).all()) for at in range(0, t.numel(), step))


def guards_intact(whole, view, written=None, fill=0xA5):
    """Nothing of `whole` outside the first `written` bytes of `view` (all of it if None) has changed from `fill`."""
    lead = view.data_ptr() - whole.data_ptr()
    end = lead + (view.numel() if written is None else written)
    return all_bytes(whole[:lead], fill) and all_bytes(whole[end:], fill)


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def _torch(a):
    import torch
    return torch.from_numpy(a) if isinstance(a, np.ndarray) else a


def periodic_equal(flat, period_bytes, periods, what="buffer", step=32):
    """flat[j * period_bytes : (j + 1) * period_bytes] equals period 0 for every j < periods (a tensor on any device, or a numpy
    array); an AssertionError names the first period that differs and the first differing byte within it."""
    flat = _torch(flat)
    assert flat.numel() >= periods * period_bytes, f"{what}: {flat.numel()} bytes, fewer than {periods} periods of {period_bytes}"
    rows = flat[: periods * period_bytes].view(periods, period_bytes)
    for j0 in range(1, periods, step):
        same = (rows[j0: j0 + step] == rows[0]).all(dim=1)
        if not bool(same.all()):
            j = j0 + int((~same).nonzero()[0, 0])
            at = int((rows[j] != rows[0]).nonzero()[0, 0])
            raise AssertionError(f"{what}: period {j} differs from period 0, first at byte {at} of the period")


def periodic_table(offsets, per_period, periods=K, what="table"):
    """offsets[0 .. periods * per_period] is period 0's table shifted by j * (the bytes of period 0) in period j: offsets[0] is 0
    and the rows of diff(offsets).view(periods, per_period) are equal.  An AssertionError names the first period that differs
    and the entry.  -> the bytes of period 0."""
    offsets = _torch(offsets)
    assert offsets.numel() >= periods * per_period + 1, f"{what}: {offsets.numel()} entries"
    assert int(offsets[0]) == 0, f"{what}: begins at {int(offsets[0])}"
    head = offsets[: periods * per_period + 1]
    rows = (head[1:] - head[:-1]).view(periods, per_period)
    same = (rows == rows[0]).all(dim=1)
    if not bool(same.all()):
        j = int((~same).nonzero()[0, 0])
        at = int((rows[j] != rows[0]).nonzero()[0, 0])
        raise AssertionError(f"{what}: period {j} differs from period 0 at entry {at}: {int(rows[j, at])} bytes, not {int(rows[0, at])}")
    return int(offsets[per_period])


def tiled_streams(payload0, offsets0, payload_tail, offsets_tail, periods=K, offset=0, device="cuda", fill=0xA5, guard=64):
    """A full payload and table from period 0's (made by the oracle, so that the decoders run on streams the encoder under test
    never produced): payload0 `periods` times, then the tail's streams; the table is offsets0 shifted by j * len(payload0)
    in period j, then the tail's.  -> (whole, payload view, table int64 [periods * per_period + len(offsets_tail)])."""
    import torch
    p0 = torch.from_numpy(np.ascontiguousarray(payload0, dtype=np.uint8)).to(device)
    pt = torch.from_numpy(np.ascontiguousarray(payload_tail, dtype=np.uint8)).to(device)
    o0 = torch.from_numpy(np.asarray(offsets0).astype(np.int64)).to(device)
    ot = torch.from_numpy(np.asarray(offsets_tail).astype(np.int64)).to(device)
    P, per = p0.numel(), o0.numel() - 1
    assert int(o0[0]) == 0 and int(o0[-1]) == P and int(ot[0]) == 0 and int(ot[-1]) == pt.numel()
    total = periods * P + pt.numel()
    whole = torch.full((guard + offset + total + guard,), fill, dtype=torch.uint8, device=device)
    view = whole[guard + offset: guard + offset + total]
    view[: periods * P].view(periods, P).copy_(p0.unsqueeze(0).expand(periods, P))
    view[periods * P:].copy_(pt)
    shift = torch.arange(periods, dtype=torch.int64, device=device).unsqueeze(1) * P
    table = torch.cat([(o0[:-1].unsqueeze(0) + shift).reshape(-1), ot + periods * P])
    assert table.numel() == periods * per + ot.numel()
    return whole, view, table


# ---- period 0 and the tail, from the oracle ------------------------------------------------------------------------------------
_streams = {}


def oracle_blocks(oracle, coder, kind="coder", block=BLOCK):
    """The oracle's streams of the tile and of the tail as the last, short block -> (payload0, offsets0, payload_tail,
    offsets_tail), computed once per coder."""
    key = (coder, kind, block)
    if key not in _streams:
        x = tile(kind)
        slots, sizes = oracle.encode_blocks(x, block, coder=coder, threads=8)
        p0, o0 = oracle.compact(slots, sizes)
        slots, sizes = oracle.encode_blocks(tail_of(x), block, coder=coder)
        pt, ot = oracle.compact(slots, sizes)
        _streams[key] = (p0, o0, pt, ot)
    return _streams[key]


def payload_bytes(oracle, coder):
    """oracle sizes of the tile * K + the tail's stream: what the compacted payload of N bytes of the coder tile holds."""
    p0, _, pt, _ = oracle_blocks(oracle, coder)
    return K * len(p0) + len(pt)


# ---- items -------------------------------------------------------------------------------------------------------------------
def item_pattern():
    """Lengths that sum to the tile: ITEM_SPECIAL (0, 1, 16, 17, 4097, 65536, 65537, 200 000) -- the five shortest in front, so
    that the tail has them too, the long ones among fill items of 64 KiB -- then one more empty item and the rest -> int64 array."""
    fill_total = T - sum(ITEM_SPECIAL)
    nfill, rest = divmod(fill_total, BLOCK)
    lengths = list(ITEM_SPECIAL[:5])
    for k in range(nfill):
        if k % 40 == 7 and k // 40 < 3:
            lengths.append(ITEM_SPECIAL[5 + k // 40])
        lengths.append(BLOCK)
    lengths += [0, rest]
    out = np.array(lengths, np.int64)
    assert int(out.sum()) == T and all(s in lengths for s in ITEM_SPECIAL)
    return out


def cut_to(lengths, nbytes):
    """The pattern's items as far as nbytes reach, the last one cut short."""
    ends = np.cumsum(lengths)
    k = int(np.searchsorted(ends, nbytes, side="left"))
    head = list(lengths[:k])
    return np.array(head + [nbytes - int(sum(head))], np.int64)


def full_lengths(pattern, tail_lengths):
    return np.concatenate([np.tile(pattern, K), tail_lengths])


def typed_pattern():
    """Typed items that sum to the tile: the superblocks (width * 64 KiB) of widths 8, 4, 2 with the predictors zigzag, delta,
    none in turn, all nine pairs three times, and one more of width 2; runs of 70 empty items in front of the second and third
    round and behind the last item -> (lengths int64, widths uint8, preds uint8).  The first item has width 8 and zigzag: the
    tail (cut_typed) is that item cut to 12345 bytes, with one tail byte."""
    pairs = [(w, p) for p in (2, 1, 0) for w in (8, 4, 2)]
    items = []
    for turn in range(3):
        if turn:
            items += [(0, 4, 1)] * 70
        items += [(w * BLOCK, w, p) for (w, p) in (pairs[turn:] + pairs[:turn])]
    items += [(T - 3 * sum(w * BLOCK for w, _ in pairs), 2, 1)] + [(0, 8, 2)] * 70
    lengths, widths, preds = (np.array([it[j] for it in items], t) for j, t in ((0, np.int64), (1, np.uint8), (2, np.uint8)))
    assert int(lengths.sum()) == T
    return lengths, widths, preds


def cut_typed(pattern, nbytes):
    lengths, widths, preds = pattern
    t = cut_to(lengths, nbytes)
    return t, widths[: len(t)].copy(), preds[: len(t)].copy()


def items_of(x, lengths):
    offs = np.concatenate([[0], np.cumsum(lengths)])
    return [x[int(offs[i]): int(offs[i + 1])] for i in range(len(lengths))]
