#!/usr/bin/env python3
"""Rate of the base-residual kernels (csrc/rcx_base.hpp) beside the plain plane filter, a device-to-device copy and the
kernels they run with: device events around the enqueued call, one process, warm-up, >= 5 rounds that alternate between
everything measured, median and min-max.  DESIGN.md section 17 quotes profiles/r15_base_rate.jsonl; never bench.py's `value`.

    python tools/base_rate.py [--out profiles/r15_base_rate.jsonl] [--repeats 5] [--bytes N]

The mt19937(12345) GiB as the source and the mt19937(54321) GiB as the base (the kernels' work does not depend on the data),
blocks of 64 KiB and of 16 KiB, everything 16-byte aligned.  Per block size, in the same rounds:
  widths 2, 4, 8: the plain split and join (rcx_planes_k, the yardstick: csrc/rcx_planes.hpp is the parent commit's file, byte
  for byte, so the library's plane kernels ARE the parent's) and the base split and join with xor, sub and subzz;
  width 1: a device-to-device copy of the same bytes (the yardstick: there is no plain kernel of width 1) and the three ops;
and the adaptive coder's encode and decode calls with the library's own per-kernel times (rcx_ctx_get_timing).
Every row is kernel time per call in milliseconds and scaled to one GiB.  The base kernels move 3n bytes where the yardsticks
move 2n, so the expectation is 1.5 times the yardstick; *_over_plain is the base kernel's median over the yardstick's median of
the same width and rounds, `margin` is 1.5 * (1 + the yardstick's own (max - min) / median in these rounds), and *_above_margin
says whether the ratio lies above it.  *_share_of_* is the kernel's time over the coder kernel's.  Nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpprcoder_amd import base, planes, rcx, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCKS = (65536, 16384)
OPS = (("xor", base.XOR), ("sub", base.SUB), ("subzz", base.SUBZZ))


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, nbytes, moved):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_per_GiB": round(med * GIB / nbytes, 4),
            "GBps_moved_median": round(moved * nbytes / 1e6 / med, 1), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_base_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    src, ref, mid, out = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(4))
    assert all(r.data_ptr() % 16 == 0 for r in (src, ref, mid, out))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())
    ref.copy_(torch.from_numpy(workloads.uniform(n, 54321)).cuda())

    rows = []
    for block in BLOCKS:
        things = {}
        for width in (2, 4, 8):
            things[f"split_plain_w{width}"] = lambda width=width: planes.split_device(ctx, src, width, block, mid)
            things[f"join_plain_w{width}"] = lambda width=width: planes.join_device(ctx, mid, width, block, out)
        things["split_plain_w1"] = lambda: mid.copy_(src)  # the yardstick of width 1: a device-to-device copy, either way
        things["join_plain_w1"] = lambda: out.copy_(mid)
        for width in base.WIDTHS:
            for name, op in OPS:
                things[f"split_{name}_w{width}"] = lambda width=width, op=op: base.split_device(ctx, src, ref, width, block, op, mid)
                things[f"join_{name}_w{width}"] = lambda width=width, op=op: base.join_device(ctx, mid, ref, width, block, op, out)
        nb = rcx.block_count(n, block)
        dst = torch.zeros(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
        offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
        back = torch.zeros(n, dtype=torch.uint8, device="cuda")
        things["encode"] = lambda: ctx.encode_blocks_device(src, block, dst, offs)
        things["decode"] = lambda: ctx.decode_blocks_device(dst, dst.numel(), offs, n, block, back)

        # warm-up and a check of what is measured: join(split(x)) = x for every width and op, decode(encode(x)) = x
        for width in base.WIDTHS:
            for name in ("plain",) + tuple(name for name, _ in OPS):
                for _ in range(2):
                    things[f"split_{name}_w{width}"]()
                    things[f"join_{name}_w{width}"]()
                ctx.sync_status()
                assert torch.equal(out, src), (block, width, name)
                out.zero_()
        for _ in range(2):
            things["encode"]()
            things["decode"]()
        ctx.sync_status()
        assert torch.equal(back, src)

        ms = {k: [] for k in things}
        kernels = {k: [] for k in ("encode", "scatter", "decode")}
        ctx.set_timing(True)
        ctx.get_timing(reset=True)
        for _ in range(args.repeats):  # one of each per round, in turn (a join always behind the split whose output it reads)
            for name, fn in things.items():
                ms[name].append(once(fn))
                if name in ("encode", "decode"):
                    ctx.sync_status()
                    t = ctx.get_timing(reset=True)
                    for k in (("encode", "scatter") if name == "encode" else ("decode",)):
                        kernels[k].append(t[k]["ms"])
        ctx.set_timing(False)

        yard = {k: stats(v, n, 1) for k, v in kernels.items() if v}
        for width in base.WIDTHS:
            plain = {what: stats(ms[f"{what}_plain_w{width}"], n, 2) for what in ("split", "join")}
            rows.append({"part": "plain", "kernel": "rcx_planes_k" if width > 1 else "device-to-device copy", "bytes": n, "block": block, "width": width,
                         "data": "uniform mt19937(12345)", **plain})
            for name, _ in OPS:
                row = {"part": "base", "kernel": "rcx_base_k", "op": name, "bytes": n, "block": block, "width": width,
                       "data": "uniform mt19937(12345) against uniform mt19937(54321)"}
                for what, coder in (("split", "encode"), ("join", "decode")):
                    s = row[what] = stats(ms[f"{what}_{name}_w{width}"], n, 3)
                    p = plain[what]
                    row[what + "_over_plain"] = round(s["ms_median"] / p["ms_median"], 3)
                    row[what + "_margin"] = round(1.5 * (1 + (p["ms_max"] - p["ms_min"]) / p["ms_median"]), 3)
                    row[what + "_above_margin"] = bool(row[what + "_over_plain"] > row[what + "_margin"])
                    row[f"{what}_share_of_{coder}"] = round(s["ms_median"] / yard[coder]["ms_median"], 4)
                rows.append(row)
        rows.append({"part": "yardsticks", "bytes": n, "block": block, "coder": "adaptive", "what": "the library's own event pairs around its kernels, same rounds",
                     "kernels": yard, "calls": {k: stats(ms[k], n, 1) for k in ("encode", "decode")}})
        del dst, offs, back
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
