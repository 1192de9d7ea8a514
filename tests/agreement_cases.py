"""The checks behind the oracle-vs-reference-build tests (test_against_reference_build, test_rans_against_reference_build,
test_reference_build_agrees), as generators of (key, result) for one checker.  tests/golden/make_golden_agreement.py runs
them over the real reference build and stores a digest of every result (tests/golden/reference_agreement.json); the tests
run them over the oracle and compare with those digests, and, where oracle/_ref is present, with the reference build's own
results as well.  A result is a tuple of ints, bools and bytes, so two checkers' results compare with ==."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from cpprcoder_amd import workloads

STORED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_agreement.json")


def stored(part: str) -> dict:
    """The reference build's digests of one check ("adaptive", "rans", "bwt" or "damaged"), key -> digest."""
    with open(STORED) as f:
        return json.load(f)[part]


def digest(result) -> str:
    """sha256 of a result, bytes standing as their own sha256 (results can be a few MiB)."""
    def plain(x):
        if isinstance(x, (bytes, bytearray)):
            return "sha256:" + hashlib.sha256(bytes(x)).hexdigest()
        if isinstance(x, (tuple, list)):
            return [plain(y) for y in x]
        if isinstance(x, (bool, np.bool_)):
            return bool(x)
        if isinstance(x, (int, np.integer)):
            return int(x)
        raise TypeError(f"not a result: {type(x)}")
    return hashlib.sha256(json.dumps(plain(result)).encode()).hexdigest()


def agree(want: dict, mine, theirs=None) -> None:
    """Every (key, result) of `mine` (the oracle's run of a check) has the stored digest want[key] and, when `theirs` (the
    reference build's run of the same check) is given, equals its result; all of want's keys come up."""
    seen = 0
    for key, got in mine:
        assert key in want and digest(got) == want[key], key
        if theirs is not None:
            ref_key, ref_got = next(theirs)
            assert (ref_key, ref_got) == (key, got), key
        seen += 1
    assert seen == len(want)


def adaptive(chk):
    """The adaptive and static range coders (cpprcoder.h): one-shot, capped sink, chunked, damaged streams, block tables."""
    rs = np.random.RandomState(2024)
    cases = [workloads.uniform(5000, 1), workloads.zipf(70000, 2), workloads.runs(150000, 3), workloads.canterbury_tiled(100000)[7:],
             np.zeros(1, np.uint8), np.full(300000, 255, np.uint8)]
    for _ in range(40):
        n = int(rs.randint(0, 3000))
        alpha = int(rs.randint(1, 257))
        cases.append(rs.randint(0, alpha, size=n).astype(np.uint8))
    for i, v in enumerate(cases):
        enc = chk.adaptive_encode(v)
        yield f"{i}/adaptive_encode", enc
        yield f"{i}/static_encode", chk.static_encode(v)
        comp = enc[1]
        yield f"{i}/adaptive_decode", chk.adaptive_decode(comp, max(len(v), 1))
        for cap in (len(comp) // 2, 16):
            yield f"{i}/adaptive_encode cap={cap}", chk.adaptive_encode(v, sink_capacity=cap)
        for piece in (0, 333):
            yield f"{i}/adaptive_encode_chunked piece={piece}", chk.adaptive_encode_chunked(v, piece)
        # corrupt / random streams must decode to the same bytes and status too
        junk = rs.randint(0, 256, size=max(len(comp), 12)).astype(np.uint8)
        junk[:4] = np.frombuffer(np.uint32(min(len(v), 500)).tobytes(), np.uint8)
        yield f"{i}/adaptive_decode junk", chk.adaptive_decode(junk, 600)
    data = workloads.zipf(1 << 20, 9)
    for block in (4096, 65536):
        slots, sizes = chk.encode_blocks(data, block, threads=4)
        yield f"encode_blocks block={block}", (sizes.tobytes(), slots.tobytes())


def rans(chk):
    """The rANS coders (cppans.h, one state and eight): the stream, and what decoding it gives."""
    rs = np.random.RandomState(77)
    cases = [workloads.uniform(5000, 1), workloads.zipf(70000, 2), workloads.runs(150000, 3), workloads.canterbury_tiled(100000)[7:],
             np.zeros(1, np.uint8), np.full(30000, 255, np.uint8)]
    for _ in range(120):
        n = int(rs.randint(1, 3000))
        cases.append(rs.randint(0, int(rs.randint(1, 257)), size=n).astype(np.uint8))
    for n in range(1, 24):  # fewer symbols than states
        cases.append(rs.randint(0, 256, size=n).astype(np.uint8))
    for i, v in enumerate(cases):
        for simd in (False, True):
            comp = chk.rans_encode(v, simd)
            yield f"{i}/simd={simd}/encode", (comp,)
            back = chk.rans_decode(comp, len(v), simd)
            assert back == (True, v.tobytes()), (chk.kind, len(v), simd)
            yield f"{i}/simd={simd}/decode", back


BWT_NAMES = ("random 2 blocks + tail", "four letters", "repeat of 5000", "period 16384 (seed 19, 256 symbols)",
             "three blocks: periodic, random, zeros")


def bwt(chk, inputs):
    """The block sort (blksort.h): BlkSort::encode of some tests/bwt_cases.py inputs, and decode of what it wrote."""
    for name in BWT_NAMES:
        enc = chk.bwt_encode(inputs[name], threads=4)
        yield f"{name}/encode", (enc.tobytes(),)
        yield f"{name}/decode", (chk.bwt_decode(enc).tobytes(),)


def damaged(chk):
    """Damaged streams the reference decodes without running dry (a RandomState of its own, so that the other checks' keys
    and digests stay as they are): the static coder's payload flips and count edits that keep the total nonzero
    (cpprcoder.h:460-535), and the rANS coders' payload flips with the table intact (cppans.h:532-564, :609-649).  Every
    stream is followed by random bytes, so that no decoder reads past its input.  Left out, as the reference leaves them
    undefined: a zero total, a bad rANS table, a payload that runs dry."""
    rs = np.random.RandomState(31337)
    cases = [workloads.uniform(5000, 21), workloads.zipf(40000, 22), workloads.canterbury_tiled(30000)[3:], workloads.runs(20000, 23)]
    for _ in range(12):
        n = int(rs.randint(1, 4000))
        cases.append(rs.randint(0, int(rs.randint(2, 257)), size=n).astype(np.uint8))
    for i, v in enumerate(cases):
        pad = rs.randint(0, 256, size=len(v) + 2048).astype(np.uint8)
        comp = np.frombuffer(chk.static_encode(v)[1], np.uint8)
        for kind in ("flips", "count to 0", "count moved"):
            s = np.concatenate([comp, pad])
            if kind == "flips":
                for _ in range(1 + i % 3):
                    s[int(rs.randint(517, max(len(comp), 518)))] ^= int(rs.randint(1, 256))
            else:
                counts = s[4:516].view("<u2").copy()
                used = np.nonzero(counts)[0]
                if len(used) < 2:
                    continue
                a, b = (int(x) for x in rs.choice(used, 2, replace=False))
                if kind == "count moved":
                    counts[b] = min(int(counts[b]) + int(counts[a]), 0xFFFF)
                counts[a] = 0
                s[4:516] = counts.view(np.uint8)
            yield f"{i}/static_decode {kind}", chk.static_decode(s, max(len(v), 1))
        for simd in (False, True):
            comp = np.frombuffer(chk.rans_encode(v, simd), np.uint8)
            s = np.concatenate([comp, pad])
            for _ in range(1 + i % 4):
                s[int(rs.randint(1032 + 4, max(len(comp), 1032 + 5)))] ^= int(rs.randint(1, 256))
            yield f"{i}/simd={simd}/decode flips", chk.rans_decode(s, len(v), simd)
