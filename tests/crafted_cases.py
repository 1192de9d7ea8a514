"""One registry of the crafted inputs: every adversarial builder the GPU tests aim at a kernel's switch points, by family, so
that the same bytes can be run through the oracle, the reference build and the kernels (tests/agreement_cases.py,
tests/test_oracle_crafted.py, tests/test_gpu_reference_digests.py).  Not a test file.  It imports the builders and copies
none; it needs numpy and the oracle (decode cases are streams the oracle made, then damaged), no GPU and no torch.

A case is Case(key, coder, kind, data, n): `coder` is 0 .. 3 (cpprcoder_amd.rcx.CODER_*) or "bwt"; `kind` says what is done
with `data`:
  "encode"         data = n symbols (for "bwt": one block of 32768 bytes) -> the stream;
  "decode"         data = a stream, followed by seeded bytes where it is damaged, of n symbols, decoded as one block of n
                   (for "bwt": one encoded block of 32770 bytes) -> (every symbol came out, the bytes if so);
  "stream_decode"  the adaptive coder only: data decoded into a bounded sink of `n` bytes -> (status, request size, bytes).
Keys are stable: a family's name, the builder's parameters.  case_key(c) is the key under which a case's result is stored.

Left out, because the reference leaves the result undefined (none of them is an encode, and for each the GPU tests assert
RCX_E_CORRUPT alone, never bytes):
  * the static coder's symbol of count 0 -- gpu_support.COUNT0, the one damaged kind that is skipped: range becomes 0
    (cpprcoder.h:500-505) and the renormalisation (cpprcoder.h:506-513) shifts bytes in for ever, past the end of its
    input.  (Every stream of static_cases.aimed_streams decodes, the half-zero table's included: all are kept.)  A static
    total of 0 (every count edited to 0) divides by zero at cpprcoder.h:500 and is built by no test;
  * a bad rANS table: cppans.h:532-564 and :609-649 read the cumulative counts unchecked and index their symbol table
    with them; no crafted builder makes one;
  * a static or rANS payload that runs dry, truncated streams of those coders included: their decoders take a pointer and
    no end (cpprcoder.h:506-513, cppans.h:540-560, :617-645) and read past the stream.  The adaptive coder's truncated
    streams are kept: its decoder is bounded by the size it is handed and answers with a status and a request size.

Not compared, and why.  The halving family holds the long inputs one-shot, encoded in constant pieces of
resumable_cases.HALVING_PIECE (the 16th piece ends with the halving symbol) and decoded in constant pieces of
CHUNKED_PIECE; the call sizes of resumable_cases.around_halving -- a boundary right before, a call that is nothing but,
and a boundary right behind the halving symbol -- are not held to the reference: the checkers' chunked calls take one
constant piece size, and pieces of differing sizes would need a new export of the reference shim.  tests/test_gpu_resumable.py
holds the kernels to the oracle at those boundaries.  resumable_cases.interleaved_inputs is ordinary data (workload
slices), which tests/golden/reference_agreement.json covers, and is not listed here.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import adaptive_cases
import adaptive_walk
import bwt_cases
import bwt_inverse_cases
import carry_runs
import damaged_cases
import golden_cases
import oracle_lib
import rans_cases
import resumable_cases
import static_cases
from cpprcoder_amd import workloads

ADAPTIVE, STATIC, RANS, RANS8 = 0, 1, 2, 3
CODER_NAMES = {ADAPTIVE: "adaptive", STATIC: "static", RANS: "rans", RANS8: "rans8", "bwt": "bwt"}


class Case(NamedTuple):
    key: str
    coder: object   # 0 .. 3 or "bwt"
    kind: str       # "encode", "decode" or "stream_decode"
    data: np.ndarray
    n: int          # symbols (for "stream_decode": the sink's capacity)


def case_key(c: Case) -> str:
    return f"{c.key}/{CODER_NAMES[c.coder]}/{c.kind}"


def _enc(key, coder, data):
    data = np.ascontiguousarray(data, np.uint8)
    return Case(key, coder, "encode", data, len(data))


def _stream(chk, coder, data):
    slots, sizes = chk.encode_blocks(data, len(data), coder=coder)
    return slots[0, : int(sizes[0])].copy()


def _both(key, coder, data):
    """A valid input as an encode, and its stream (the oracle's; the encode case pins it to the reference) as a decode."""
    data = np.ascontiguousarray(data, np.uint8)
    yield _enc(key, coder, data)
    yield Case(key, coder, "decode", _stream(oracle_lib.oracle(), coder, data), len(data))


# ---- carry: a carry through a held run of 0xFF bytes (tests/carry_runs.py) ------------------------------------------------
PARITY_RUNS = [0, 3, 20, 30, 40, 70, 300, 0, 0, 45, 0, 1000]            # test_gpu_parity: block 4096, seed 100 + i
POSITION_RUNS = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 24, 33, 40]      # test_gpu_parity: seed 9000 + 100 i + k, behind `after`
POSITION_AFTER = [0, 150, 260, 515, 770, 1290, 2000, 3000]
STATIC_PARITY_RUNS = [0, 5, 20, 60, 100, 0, 45]                         # test_gpu_parity: block 8192, seed 1000 i + the first that works
CPU_RUNS, CPU_STATIC_RUNS = (3, 40, 200), (5, 60)                        # test_carry_runs: seed 7 + run; 1000 + the first that works
TRACE_RUNS = (3, 40, 300)                                                # trace_cases: seed 5 + run


def _first_static(block, run, base):
    for seed in range(50):
        try:
            return seed, carry_runs.carry_run_block_static(block, run, base + seed)
        except AssertionError:
            pass
    raise RuntimeError("no carry run found")


@functools.lru_cache(maxsize=None)
def carry_blocks():
    """-> [(key, "adaptive" or "static": the coder the run was steered for, block)]; the (block, run, seed) triples of
    test_gpu_parity.py, test_carry_runs.py and trace_cases.py.  A seed for which the builder finds no run is left out as
    the tests leave it out."""
    out = []
    for i, r in enumerate(PARITY_RUNS):
        if r:
            out.append((f"run {r} seed {100 + i}", "adaptive", carry_runs.carry_run_block(4096, r, 100 + i)))
    for i, run in enumerate(POSITION_RUNS):
        for k, after in enumerate(POSITION_AFTER):
            try:
                out.append((f"run {run} seed {9000 + 100 * i + k} after {after}", "adaptive",
                            carry_runs.carry_run_block(4096, run, 9000 + 100 * i + k, after)))
            except AssertionError:
                continue
    for run in CPU_RUNS:
        out.append((f"run {run} seed {7 + run}", "adaptive", carry_runs.carry_run_block(4096, run, 7 + run)))
    for run in TRACE_RUNS:
        out.append((f"run {run} seed {5 + run}", "adaptive", carry_runs.carry_run_block(4096, run, 5 + run)))
    for i, r in enumerate(STATIC_PARITY_RUNS):
        if r:
            seed, block = _first_static(8192, r, 1000 * i)
            out.append((f"static run {r} seed {1000 * i + seed}", "static", block))
    for run in CPU_STATIC_RUNS:
        seed, block = _first_static(8192, run, 1000)
        out.append((f"static run {run} seed {1000 + seed}", "static", block))
    once = {key: (key, kind, block) for key, kind, block in out}   # (run 5 from seed 1000 on is in both tests)
    return list(once.values())


def carry():
    """Every block by both range coders (a run steered for one coder is ordinary data to the other)."""
    for key, _, block in carry_blocks():
        yield _enc(f"carry/{key}", ADAPTIVE, block)
        yield _enc(f"carry/{key}", STATIC, block)


# ---- static: large totals and the 16-bit squeeze (tests/static_cases.py) -----------------------------------------------------
ULPS = (0, 1, -1)


NATURAL_STREAM = "static/natural stream"   # 2^24 bytes: past RCX_MAX_BLOCK, a single stream to the kernels


@functools.lru_cache(maxsize=None)
def static_encodes():
    """The blocks squeeze_points() is pinned on (test_static_cases_cpu): the ladder, the block with two squeezes and the two
    natural inputs.  Apart from the decodes, which take the oracle some seconds to make."""
    ladder, twice = static_cases.squeeze_ladder()
    out = [_enc(f"static/ladder/{name}", STATIC, block) for name, block, _ in ladder]
    out.append(_enc("static/ladder/two squeezes", STATIC, twice))
    out.append(_enc("static/natural block", STATIC, static_cases.natural_block()))
    out.append(_enc(NATURAL_STREAM, STATIC, static_cases.natural_stream()))
    return tuple(out)


def static():
    yield from static_encodes()
    for name in static_cases.tables():
        for b, (_, stream) in enumerate(static_cases.crafted_blocks(name)):
            yield Case(f"static/crafted/{name}/{b}", STATIC, "decode", stream, static_cases.BLOCK)
        for ulp in ULPS:  # (every aimed stream decodes, the half-zero table's too: test_static_cases_cpu asserts it)
            for i, s in enumerate(static_cases.aimed_streams(name, ulp)):
                yield Case(f"static/aimed/{name}/ulp {ulp:+d}/{i}", STATIC, "decode", s, 4096)


# ---- rans: the model's steal loop, the output rings, wave mixes (tests/rans_cases.py) ------------------------------------------
def rans_blocks():
    """name -> block: block_cases() (victim_cases with its tie_counts blocks, singletons, dense_rare, one_symbol, all_256)
    and the rare_item items of the GPU tests' length sets (test_gpu_rans_shapes.mixed_items: every third item)."""
    out = dict(rans_cases.block_cases())
    sets = [(name, lengths, 40 + len(name)) for name, lengths in rans_cases.LENGTH_SETS.items()]
    sets.append(("mixed, reversed", rans_cases.WAVE_MIXED, 77))
    for name, lengths, seed in sets:
        for k, n in enumerate(lengths):
            if k % 3 == 2:
                out[f"rare_item({n}, {seed + k}) of {name}"] = rans_cases.rare_item(n, seed + k)
    return out


def rans():
    for name, block in rans_blocks().items():
        for coder in (RANS, RANS8):
            yield from _both(f"rans/{name}", coder, block)


# ---- bwt: the forward kernel's switch points, the inverse kernel's (tests/bwt_cases.py, tests/bwt_inverse_cases.py) -----------
PLANTED = ((40, 5639, 0), (40, 1543, 0), (40, 519, 0), (40, 9, 1030), (40, 8, 348))   # test_bwt_cases_cpu's (seed, twice, thrice)


@functools.lru_cache(maxsize=None)
def bwt_blocks():
    """name -> a block of 32768 bytes.  The ladders, the run-keyed blocks (aligned_runs and tied_runs among them, as built
    and turned), planted blocks, and every periodic block of bwt_cases.cases()."""
    out = {}
    for limit in bwt_cases.LIST_LENGTHS:
        for i, b in enumerate(bwt_cases.open_ladder(limit)):
            out[f"open_ladder({limit})/{i}"] = b
    for i, b in enumerate(bwt_cases.runny_ladder()):
        out[f"runny_ladder/{i}"] = b
    for name, b in bwt_cases.run_key_cases().items():
        out[f"run keys/{name}"] = b
    for seed, twice, thrice in PLANTED:
        out[f"planted({seed}, {twice}, {thrice})"] = bwt_cases.planted(seed, twice, thrice)
    for name, b in bwt_cases.cases().items():
        if name.startswith("period ") and len(b) == bwt_cases.BLOCK:
            out[f"periodic/{name}"] = b
    return out


def bwt_encoded(chk, blocks, threads=8):
    """Every block's encoding, in order.  A block a call, handed out to `threads` threads as they come free (ctypes drops
    the GIL for a call): a block full of ties takes either checker 1 - 4 s, most others milliseconds."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(lambda b: chk.bwt_encode(b), blocks))


@functools.lru_cache(maxsize=None)
def oracle_encoded():
    """The oracle's encoding of every block of bwt_blocks(), made once (some ten seconds)."""
    return bwt_encoded(oracle_lib.oracle(), list(bwt_blocks().values()))


def bwt(encoded=True):
    """`encoded`: also the decode of every forward block's encoding (the oracle's; the encode case pins it to the reference)."""
    blocks = bwt_blocks()
    for name, b in blocks.items():
        yield _enc(f"bwt/{name}", "bwt", b)
    if encoded:
        for name, e in zip(blocks, oracle_encoded()):
            yield Case(f"bwt/{name}", "bwt", "decode", e, bwt_cases.BLOCK)
    for family, items in bwt_inverse_cases.all_cases().items():
        for name, blk in items:
            yield Case(f"bwt/inverse/{family}/{name}", "bwt", "decode", blk, bwt_cases.BLOCK)


# ---- adaptive: bursts, one-value blocks (tests/adaptive_cases.py) ---------------------------------------------------------------
def adaptive():
    for group in adaptive_cases.PASS_BURST_GROUPS:
        for b, block in enumerate(adaptive_cases.pass_burst_blocks(group)):
            yield from _both(f"adaptive/pass burst/group {group}/{b}", ADAPTIVE, block)
    for fill, seed in adaptive_cases.LONG_BURSTS:
        yield from _both(f"adaptive/long burst/{fill}", ADAPTIVE, adaptive_cases.long_burst_block(fill, seed))
    for byte in adaptive_cases.ONE_VALUE_BYTES:
        yield from _both(f"adaptive/one value/{byte}", ADAPTIVE, adaptive_cases.one_value_block(byte))
    for case in adaptive_cases.LEVEL3_CASES:
        yield from _both(f"adaptive/level 3/{case}", ADAPTIVE, adaptive_cases.level3_block(case))


# ---- damaged: targets past the table, and the kinds of damaged_cases.build() ----------------------------------------------------
PASS_POSITIONS = (0, 1, 15)
DAMAGED_SHAPES = ((4096, 100), (65536, 24))   # test_gpu_damaged: (block, nblocks), seed 100 + coder


def past_the_table_streams():
    """-> [(key, stream, n)]: test_gpu_dec_pass64's (pass, group, position) and test_gpu_dec_borrow_words' positions."""
    chk, block, out = oracle_lib.oracle(), adaptive_cases.PASS_BLOCK, []
    for which in ("first_pass", "late_pass"):
        for group in range(4):
            groups = [group] if which == "first_pass" else [4 * p + group for p in range(20, 40)]
            for position in PASS_POSITIONS:
                seed = 8500 + 16 * group + position
                d = damaged_cases.Damaged(chk, workloads.by_name("zipf", 16 * block, seed), block, ADAPTIVE, seed)
                made = None
                for b in ((5 * group + 3 * position + k) % 16 for k in range(16)):
                    made = adaptive_walk.past_the_table(d, b, position, groups=groups)
                    if made is not None:
                        break
                if made is not None:   # (the first symbol of the first pass has no target past the table: the test asserts it)
                    out.append((f"{which}/group {group}/position {position}", made[0], block))
    for position, b in zip(PASS_POSITIONS, (5, 0, 15)):
        d = damaged_cases.Damaged(chk, workloads.by_name("zipf", 16 * block, 40 + position), block, ADAPTIVE, 40 + position)
        out.append((f"from group 20 on/position {position}", adaptive_walk.past_the_table(d, b, position)[0], block))
    return out


@functools.lru_cache(maxsize=None)
def _built(coder, block, nblocks):
    return damaged_cases.build(oracle_lib.oracle(), coder, block, nblocks, 100 + coder)


def damaged():
    for key, stream, n in past_the_table_streams():
        yield Case(f"damaged/past the table/{key}", ADAPTIVE, "decode", stream, n)
    for block, nblocks in DAMAGED_SHAPES:
        for coder in (ADAPTIVE, STATIC, RANS, RANS8):
            d = _built(coder, block, nblocks)
            for b in sorted(d.kind):
                if d.kind[b] != damaged_cases.COUNT0:   # (left out: see the module's text)
                    yield Case(f"damaged/block {block}/{d.kind[b]}", coder, "decode", d.rows[b], d.length(b))


# ---- truncations: the adaptive coder's streams cut short ------------------------------------------------------------------------
CUTS = (1, 4, 5, 16)


def truncations():
    """The blocks test_gpu_damaged cuts (nblocks / 2 + 2, + 4, + 6, + 8 by 1, 4, 5 and 16 bytes), as a block of the block
    call and as a single stream into a bounded sink."""
    for block, nblocks in DAMAGED_SHAPES:
        d = _built(ADAPTIVE, block, nblocks)
        for j, k in enumerate(CUTS):
            b = d.nblocks // 2 + 2 + 2 * j
            assert b not in d.kind
            cut = d.orig[b][:-k].copy()
            yield Case(f"truncations/block {block}/cut by {k}", ADAPTIVE, "decode", cut, d.length(b))
            yield Case(f"truncations/block {block}/cut by {k}", ADAPTIVE, "stream_decode", cut, (d.length(b) + 15) & ~15)


# ---- halving: the resumable coders' inputs (tests/resumable_cases.py) ----------------------------------------------------------
LONG = (resumable_cases.LONG_UNIFORM, resumable_cases.LONG_MIN_ZIPF)   # 2^24 symbols and more: the table is halved


@functools.lru_cache(maxsize=None)
def halving_inputs():
    out = {label: golden_cases.LONG_ADAPTIVE[label]() for label in LONG}
    out["loop_input"] = resumable_cases.loop_input()
    out["backlog_input"] = resumable_cases.backlog_input()
    out["carry_input"] = resumable_cases.carry_input()
    return out


def halving():
    """Encodes, and the oracle's stream of each input as a single stream into a sink of n + 64 bytes."""
    chk = oracle_lib.oracle()
    for label, v in halving_inputs().items():
        yield _enc(f"halving/{label}", ADAPTIVE, v)
        comp = np.frombuffer(chk.adaptive_encode(v)[1], np.uint8)
        yield Case(f"halving/{label}", ADAPTIVE, "stream_decode", comp, len(v) + 64)


# family -> the builders it takes its cases from (tests/test_oracle_crafted.py holds this to a list of what the GPU tests use)
BUILDERS = {
    "carry": ("carry_runs.carry_run_block", "carry_runs.carry_run_block_static"),
    "static": ("static_cases.squeeze_ladder", "static_cases.natural_block", "static_cases.natural_stream",
               "static_cases.crafted_blocks", "static_cases.aimed_streams"),
    "rans": ("rans_cases.block_cases", "rans_cases.victim_cases", "rans_cases.tie_counts", "rans_cases.singletons",
             "rans_cases.dense_rare", "rans_cases.one_symbol", "rans_cases.all_256", "rans_cases.rare_item"),
    "bwt": ("bwt_cases.open_ladder", "bwt_cases.runny_ladder", "bwt_cases.run_key_cases", "bwt_cases.aligned_runs",
            "bwt_cases.tied_runs", "bwt_cases.planted", "bwt_cases.periodic", "bwt_inverse_cases.all_cases"),
    "adaptive": ("adaptive_cases.pass_burst_blocks", "adaptive_cases.long_burst_block", "adaptive_cases.one_value_block",
                 "adaptive_cases.level3_block"),
    "damaged": ("adaptive_walk.past_the_table", "damaged_cases.build"),
    "truncations": ("damaged_cases.build",),
    "halving": ("golden_cases.LONG_ADAPTIVE", "resumable_cases.loop_input", "resumable_cases.backlog_input", "resumable_cases.carry_input"),
}

FAMILIES = {"carry": carry, "static": static, "rans": rans, "bwt": bwt, "adaptive": adaptive, "damaged": damaged,
            "truncations": truncations, "halving": halving}


@functools.lru_cache(maxsize=None)
def cases(family):
    """A family's cases, made once and never written to (the static family's streams take the oracle some seconds)."""
    return tuple(FAMILIES[family]())


def encodes(family):
    """A family's encode cases alone (the static family's without making its decode streams)."""
    return static_encodes() if family == "static" else tuple(c for c in cases(family) if c.kind == "encode")


def keys(family):
    return [case_key(c) for c in cases(family)]
