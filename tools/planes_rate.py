#!/usr/bin/env python3
"""Rate of the byte-plane filter (csrc/rcx_planes.hpp) beside the kernels it runs with: device events around the enqueued
call, one process, warm-up, >= 5 repeats that alternate between everything measured, median and min-max.  DESIGN.md section
11 quotes profiles/r07_planes_rate.jsonl; never bench.py's `value`.

    python tools/planes_rate.py [--out profiles/r07_planes_rate.jsonl] [--repeats 7] [--bytes N]

The mt19937(12345) GiB (bench.py's buffer), blocks of 64 KiB:
  split and join for width 2, 4 and 8, source and destination 16-byte aligned;
  the same at width 2 with source and destination 1 byte off;
  and in the same rounds the adaptive coder's encode and decode calls with the library's own per-kernel times
  (rcx_ctx_get_timing): encode, rcx_scatter_k -- the project's streaming yardstick, which moves the bytes the filter moves
  (n read, n written) -- and decode.
Every row is kernel time per call in milliseconds and scaled to one GiB.  *_over_scatter is the filter's median over
scatter's from this file; *_share_of_* is the filter's time over the coder kernel's.  Nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpprcoder_amd import planes, rcx, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCK = 65536


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_per_GiB": round(med * GIB / nbytes, 4),
            "GBps_moved_median": round(2 * nbytes / 1e6 / med, 1), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_planes_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--only", default=None, help="diagnostic: run just this one measurement (e.g. split_w2) for a counter pass")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    room = [torch.zeros(n + 16, dtype=torch.uint8, device="cuda") for _ in range(3)]
    assert all(r.data_ptr() % 16 == 0 for r in room)
    room[0][:n].copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())
    room[0][1: 1 + n].copy_(room[0][:n].clone())  # the same bytes one byte off as well (the last byte of the aligned view differs: no matter)

    def views(off):
        return [r[off: off + n] for r in room]

    configs = [(2, 0), (4, 0), (8, 0), (2, 1)]  # (width, bytes off a 16-byte border)
    things = {}
    for width, off in configs:
        src, mid, out = views(off)
        tag = f"w{width}" + ("_off1" if off else "")
        things["split_" + tag] = lambda src=src, mid=mid, width=width: planes.split_device(ctx, src, width, BLOCK, mid)
        things["join_" + tag] = lambda mid=mid, out=out, width=width: planes.join_device(ctx, mid, width, BLOCK, out)
    src = room[0][:n]
    nb = rcx.block_count(n, BLOCK)
    dst = torch.zeros(rcx.encode_bound(n, BLOCK), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    things["encode"] = lambda: ctx.encode_blocks_device(src, BLOCK, dst, offs)
    things["decode"] = lambda: ctx.decode_blocks_device(dst, dst.numel(), offs, n, BLOCK, back)
    if args.only:
        need = {"join": ["split_" + args.only.split("_", 1)[1]], "decode": ["encode"]}.get(args.only.split("_")[0], [])
        things = {k: things[k] for k in need + [args.only]}

    # warm-up and a check of what is measured: join(split(x)) = x at every width and offset, decode(encode(x)) = x
    for _ in range(2):
        for fn in things.values():
            fn()
    ctx.sync_status()
    if not args.only:
        for width, off in configs:
            s, m, o = views(off)
            planes.split_device(ctx, s, width, BLOCK, m)
            planes.join_device(ctx, m, width, BLOCK, o)
            assert torch.equal(o, s), (width, off)
        assert torch.equal(back, src)

    ms = {k: [] for k in things}
    kernels = {k: [] for k in ("encode", "scatter", "decode")}
    ctx.set_timing(True)
    ctx.get_timing(reset=True)
    for _ in range(args.repeats):  # one of each per round, in turn
        for name, fn in things.items():
            ms[name].append(once(fn))
            if name in ("encode", "decode"):
                ctx.sync_status()
                t = ctx.get_timing(reset=True)
                for k in (("encode", "scatter") if name == "encode" else ("decode",)):
                    kernels[k].append(t[k]["ms"])
    ctx.set_timing(False)

    rows = []
    yard = {k: stats(v, n) for k, v in kernels.items() if v}
    for width, off in configs:
        tag = f"w{width}" + ("_off1" if off else "")
        if "split_" + tag not in ms and "join_" + tag not in ms:
            continue
        row = {"part": "planes", "bytes": n, "block": BLOCK, "width": width, "bytes_off_16": off, "data": "uniform mt19937(12345)"}
        for what, coder in (("split", "encode"), ("join", "decode")):
            if what + "_" + tag not in ms:
                continue
            s = row[what] = stats(ms[what + "_" + tag], n)
            if "scatter" in yard:
                row[what + "_over_scatter"] = round(s["ms_median"] / yard["scatter"]["ms_median"], 3)
            if coder in yard:
                row[f"{what}_share_of_{coder}"] = round(s["ms_median"] / yard[coder]["ms_median"], 4)
        rows.append(row)
    if yard:
        rows.append({"part": "yardsticks", "bytes": n, "block": BLOCK, "coder": "adaptive", "what": "the library's own event pairs around its kernels, same rounds",
                     "kernels": yard, "calls": {k: stats(ms[k], n) for k in ("encode", "decode") if k in ms}})
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
