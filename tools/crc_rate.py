#!/usr/bin/env python3
"""Rate of the CRC-32 kernel (csrc/rcx_crc.hpp) beside the kernels it runs with: device events around the enqueued call,
warm-up, >= 5 repeats, median and min-max.  DESIGN.md section 10 quotes profiles/r06_crc_rate.jsonl; never bench.py's
`value`.

    python tools/crc_rate.py [--out profiles/r06_crc_rate.jsonl] [--repeats 7] [--bytes N]

  blocks   the mt19937(12345) GiB (bench.py's buffer) in blocks of 4 KiB, 64 KiB and 1 MiB: rcx_crc32_blocks_device and
           rcx_crc32_verify_blocks_device, and from the same process and buffer the adaptive coder's encode and decode calls
           with the library's own per-kernel times (rcx_ctx_get_timing): encode, scan, rcx_scatter_k -- the project's
           streaming yardstick, DESIGN.md section 3.3 -- and decode.  crc_share_of_* = the CRC time over the coder's.
  ragged   lengths log-uniform over 4 KiB .. 256 KiB summing to the same bytes, starts unaligned (tools/items_rate.py part C):
           rcx_crc32_items_device beside the item encode and decode calls.
  small    200 000 items of 64 bytes: one wave per item, a rate question the issue left open.
Every row is kernel time per call in milliseconds and scaled to one GiB; nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import rcx, workloads  # noqa: E402

GIB = float(1 << 30)


def timed(fn, repeats, warmup=2):
    """-> list of milliseconds (device events on the current stream)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_per_GiB": round(med * GIB / nbytes, 4),
            "GBps_median": round(nbytes / 1e6 / med, 1), "repeats": len(ms)}


def kernel_times(ctx, fn, repeats, names, nbytes):
    """The library's own event pairs around its kernels (rcx_ctx_set_timing) -> {name: ms per call and per GiB}."""
    fn()
    ctx.sync_status()
    ctx.set_timing(True)
    ctx.get_timing(reset=True)
    for _ in range(repeats):
        fn()
    ctx.sync_status()
    t = ctx.get_timing(reset=True)
    ctx.set_timing(False)
    return {k: {"ms_mean": round(t[k]["ms"] / repeats, 4), "ms_per_GiB": round(t[k]["ms"] / repeats * GIB / nbytes, 4),
                "launches_per_call": t[k]["launches"] // repeats} for k in names}


def part_blocks(args, emit, src, n):
    ctx = rcx.Context(0)
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for block in (4096, 65536, 1 << 20):
        nb = rcx.block_count(n, block)
        crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
        dst = torch.zeros(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
        offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
        store = timed(lambda: ctx.crc32_blocks_device(src, block, crc), args.repeats)
        verify = timed(lambda: ctx.verify_blocks_device(src, block, crc), args.repeats)
        ctx.sync_status()
        enc = timed(lambda: ctx.encode_blocks_device(src, block, dst, offs), args.repeats)
        ctx.sync_status()
        total = int(offs[-1])
        dec = timed(lambda: ctx.decode_blocks_device(dst, total, offs, n, block, out), args.repeats)
        ctx.sync_status()
        assert torch.equal(out, src)
        kt = kernel_times(ctx, lambda: ctx.encode_blocks_device(src, block, dst, offs), args.repeats, ("encode", "scan", "scatter"), n)
        kt.update(kernel_times(ctx, lambda: ctx.decode_blocks_device(dst, total, offs, n, block, out), args.repeats, ("decode",), n))
        s, v, e, d = stats(store, n), stats(verify, n), stats(enc, n), stats(dec, n)
        emit({"part": "blocks", "bytes": n, "block": block, "blocks": nb, "data": "uniform mt19937(12345)", "crc32_store": s, "crc32_verify": v,
              "adaptive_encode_call": e, "adaptive_decode_call": d, "kernels": kt,
              "crc_share_of_encode": round(s["ms_median"] / e["ms_median"], 4), "crc_share_of_decode": round(v["ms_median"] / d["ms_median"], 4),
              "crc_over_scatter": round(s["ms_median"] / kt["scatter"]["ms_mean"], 3) if kt["scatter"]["ms_mean"] else None})
        del dst
    ctx.close()


def part_ragged(args, emit, src, n):
    rs = np.random.RandomState(2025)
    lengths, left = [], n
    while left > 0:
        k = min(int(np.exp(rs.uniform(np.log(4096), np.log(262144)))), left)
        lengths.append(k)
        left -= k
    soffs = rcx.item_offsets(lengths)
    ctx = rcx.Context(0)
    crc = torch.zeros(len(lengths), dtype=torch.int32, device="cuda")
    dst = torch.zeros(rcx.encode_items_bound(soffs), dtype=torch.uint8, device="cuda")
    ioffs = torch.zeros(len(soffs), dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    store = timed(lambda: ctx.crc32_items_device(src, soffs, crc), args.repeats)
    verify = timed(lambda: ctx.verify_items_device(src, soffs, crc), args.repeats)
    ctx.sync_status()
    enc = timed(lambda: ctx.encode_items_device(src, soffs, dst, ioffs), args.repeats)
    ctx.sync_status()
    total = int(ioffs[-1])
    dec = timed(lambda: ctx.decode_items_device(dst, total, ioffs, soffs, out), args.repeats)
    ctx.sync_status()
    assert torch.equal(out, src)
    s, v, e, d = stats(store, n), stats(verify, n), stats(enc, n), stats(dec, n)
    emit({"part": "ragged", "bytes": n, "items": len(lengths), "longest": int(max(lengths)), "shortest": int(min(lengths)),
          "what": "the calls include the upload of the item tables", "crc32_store": s, "crc32_verify": v, "adaptive_encode_call": e,
          "adaptive_decode_call": d, "crc_share_of_encode": round(s["ms_median"] / e["ms_median"], 4),
          "crc_share_of_decode": round(v["ms_median"] / d["ms_median"], 4)})
    ctx.close()


def part_small(args, emit, src):
    nitems = 200_000
    soffs = rcx.item_offsets(np.full(nitems, 64))
    n = int(soffs[-1])
    ctx = rcx.Context(0)
    crc = torch.zeros(nitems, dtype=torch.int32, device="cuda")
    dst = torch.zeros(rcx.encode_items_bound(soffs), dtype=torch.uint8, device="cuda")
    ioffs = torch.zeros(nitems + 1, dtype=torch.int64, device="cuda")
    part = src[1: 1 + n]
    store = timed(lambda: ctx.crc32_items_device(part, soffs, crc), args.repeats)
    ctx.sync_status()
    enc = timed(lambda: ctx.encode_items_device(part, soffs, dst, ioffs), args.repeats)
    ctx.sync_status()
    emit({"part": "small", "items": nitems, "item_bytes": 64, "bytes": n, "what": "the calls include planning and the upload of the item tables",
          "crc32_store": stats(store, n), "adaptive_encode_call": stats(enc, n)})
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_crc_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--parts", default="blocks,ragged,small")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    n = args.bytes
    src = torch.from_numpy(workloads.uniform(n, 12345)).cuda()
    parts = args.parts.split(",")
    if "blocks" in parts:
        part_blocks(args, emit, src, n)
    if "ragged" in parts:
        part_ragged(args, emit, src, n)
    if "small" in parts:
        part_small(args, emit, src)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
