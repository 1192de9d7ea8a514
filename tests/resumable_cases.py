"""Inputs and call schedules for the tests of the resumable coders across their call boundaries (tests/test_gpu_resumable.py,
the piecewise cases of tests/test_gpu_facade.py).  Pure: numpy and the generators only, nothing here touches a GPU or the
oracle; tests/test_support_cpu.py holds what is claimed here to the CPU oracle."""
import numpy as np

import carry_runs
from cpprcoder_amd import workloads
from golden_cases import NO_HALVING

M = 1 << 32

# ---- A: the table halving (cpprcoder.h:1138) ---------------------------------------------------------------------------
H = NO_HALVING                 # after H symbols the total is 2^24: symbol H - 1 halves the table
HALVING_PIECE = 1_048_560      # H / 16: with constant pieces of this size the 16th call ends exactly at the halving
LONG_UNIFORM = "uniform(NO_HALVING+5000,11)"   # golden_cases.LONG_ADAPTIVE: 256 live symbols
LONG_MIN_ZIPF = "min(zipf(2^24+70000,5),3)"    # 252 symbols stay at count 1 through the halving
CHUNKED_PIECE = 65_521         # a prime below 64 KiB: the long stream in pieces that fall nowhere in particular


def around_halving(n):
    """Call sizes that put a boundary before, inside and after the halving symbol: [H - 1, 1, 1, the rest]."""
    assert n > H + 1
    return [H - 1, 1, 1, n - H - 1]


def split(data, sizes):
    """`data` cut into consecutive pieces of `sizes` bytes (which must add up to it)."""
    assert sum(sizes) == len(data)
    out, at = [], 0
    for s in sizes:
        out.append(data[at: at + s])
        at += s
    return out


def constant(total, piece):
    """The sizes of `total` bytes in pieces of `piece`, the last one shorter."""
    return [min(piece, total - at) for at in range(0, total, piece)]


# ---- B: the decoder's launch loop (RCX_DSTREAM_CHUNK = 2^20 symbols a launch) and its input buffer ------------------------
CHUNK = 1 << 20
LOOP_N = 5 << 19               # 2.5 Mi symbols: three launches


def loop_input():
    """Four symbol values, so that 2.5 Mi symbols make a stream of well under 1 MB."""
    return np.minimum(workloads.zipf(LOOP_N, 5), 3).astype(np.uint8)


LOOP_CAPS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK)   # each repeated with size = 0 until the stream is done
LOOP_ONE_CALL = LOOP_N + 5                              # three launches in one call


def backlog_input():
    return workloads.zipf(400_000, 5)


BACKLOG_PIECE, BACKLOG_CAP, DRAIN_CAP = 100_000, 1000, 50_000
UNEVEN_PIECES = (100_000, 1, 1, 70_000, 8)   # then the rest
UNEVEN_CAPS = (0, 1, 4096)                   # dst_cap of the feeding calls, in turn


def uneven(total):
    assert total > sum(UNEVEN_PIECES)
    return list(UNEVEN_PIECES) + [total - sum(UNEVEN_PIECES)]


# ---- C: a pending run longer than any guess of the encoder's callers ------------------------------------------------------
CARRY_N, CARRY_RUN, CARRY_SEED, CARRY_PIECE = 16384, 5000, 5005, 64
FACADE_ROOM = 3 * CARRY_PIECE + 4096   # what the facade hands rcx_estream_encode for a piece of 64 bytes


def carry_input():
    return carry_runs.carry_run_block(CARRY_N, CARRY_RUN, CARRY_SEED)


def writer_events(data):
    """The reference's delayed writer (cpprcoder.h:764-802) run over `data` with the arithmetic of carry_runs.py ->
    [(symbol index, run length, carried)]: every time a run of pending 0xFF bytes ends, by a carry (they go out as 0x00)
    or by a smaller byte (they go out as 0xFF)."""
    cnt = [1] * 256
    total, low, rng, pending = 256, 0, 0xFFFFFF00, 0
    events = []
    for i, c in enumerate(bytes(data)):
        t = rng // total
        moved = low + sum(cnt[:c]) * t
        if moved >= M:
            if pending:
                events.append((i, pending, True))
            pending = 0
        low = moved % M
        rng = cnt[c] * t
        while rng < (1 << 24):
            if (low >> 24) == 0xFF:
                pending += 1
            else:
                if pending:
                    events.append((i, pending, False))
                pending = 0
            low = (low << 8) % M
            rng <<= 8
        cnt[c] += 1
        total += 1
    return events


def state_before(data, upto):
    """-> (counts, total, low, range) of the coder before symbol `upto`."""
    cnt = [1] * 256
    total, low, rng = 256, 0, 0xFFFFFF00
    for c in bytes(data[:upto]):
        t = rng // total
        low = (low + sum(cnt[:c]) * t) % M
        rng = cnt[c] * t
        while rng < (1 << 24):
            low = (low << 8) % M
            rng <<= 8
        cnt[c] += 1
        total += 1
    return cnt, total, low, rng


def carrying_symbol(data):
    """The index of the symbol whose carry runs through the long pending run."""
    long_runs = [(i, run, carried) for i, run, carried in writer_events(data) if run >= CARRY_RUN]
    assert len(long_runs) == 1 and long_runs[0][2], long_runs
    return long_runs[0][0]


def without_the_carry(data, j=None):
    """`data` up to the carrying symbol j, then a symbol whose interval ends at or below the wrap point (no carry: the
    coded value stays below it whatever follows, so the run goes out as 0xFF bytes), then other seeded bytes
    -> (the altered input, j)."""
    if j is None:
        j = carrying_symbol(data)
    cnt, total, low, rng = state_before(data, j)
    t = rng // total
    assert low + total * t > M, "the interval does not straddle the wrap point before the carrying symbol"
    pick, cum = None, 0
    for s in range(256):
        if low + (cum + cnt[s]) * t <= M:
            pick = s     # the highest symbol that lies entirely below the wrap point
        cum += cnt[s]
    assert pick is not None and pick != int(data[j])
    tail = np.random.RandomState(CARRY_SEED + 1).randint(0, 256, len(data) - j - 1).astype(np.uint8)
    return np.concatenate([np.asarray(data[:j], np.uint8), np.array([pick], np.uint8), tail]), j


# ---- E: several objects on one context -------------------------------------------------------------------------------------
def interleaved_inputs():
    """-> [(kind, bytes, piece)]: two streams to decode and two inputs to encode, all different, 20 000 to 70 000 symbols."""
    return [("dec", workloads.zipf(70_000, 21).tobytes(), 4099),
            ("enc", workloads.uniform(20_000, 22).tobytes(), 777),
            ("dec", workloads.canterbury_files()["fields.c"] * 3, 1000),
            ("enc", workloads.zipf(45_001, 24).tobytes(), 5000)]


BLOCKS, BLOCK = 8, 4096   # the block call made between the rounds
