#!/usr/bin/env python3
"""Rate of the delta predictor's fused kernels (csrc/rcx_predict.hpp) beside the plain plane filter and the kernels they
run with: device events around the enqueued call, one process, warm-up, >= 5 rounds that alternate between everything
measured, median and min-max.  DESIGN.md section 12 quotes profiles/r08_predict_rate.jsonl; never bench.py's `value`.

    python tools/predict_rate.py [--out profiles/r08_predict_rate.jsonl] [--repeats 5] [--bytes N]

The mt19937(12345) GiB (bench.py's buffer; the kernels' work does not depend on the data), blocks of 64 KiB, everything
16-byte aligned.  Per width 2, 4 and 8, in the same rounds:
  the plain split and join (rcx_planes_k: the yardstick);
  the fused split and join with the delta and with the zigzag predictor;
and the adaptive coder's encode and decode calls with the library's own per-kernel times (rcx_ctx_get_timing): encode,
rcx_scatter_k and decode.
Every row is kernel time per call in milliseconds and scaled to one GiB.  *_over_plain is the fused kernel's median over the
plain one's of the same width; *_share_of_* is its time over the coder kernel's; `outside_plain_spread` says whether the
fused split's median lies outside the plain split's min-max by more than that spread.  Nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpprcoder_amd import predict, rcx, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCK = 65536
WIDTHS = (2, 4, 8)
PREDS = (("plain", predict.NONE), ("delta", predict.DELTA), ("zigzag", predict.ZIGZAG))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_predict_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    src, mid, out = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    assert all(r.data_ptr() % 16 == 0 for r in (src, mid, out))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())

    things = {}
    for width in WIDTHS:
        for name, pred in PREDS:
            things[f"split_{name}_w{width}"] = lambda width=width, pred=pred: predict.split_device(ctx, src, width, BLOCK, pred, mid)
            things[f"join_{name}_w{width}"] = lambda width=width, pred=pred: predict.join_device(ctx, mid, width, BLOCK, pred, out)
    nb = rcx.block_count(n, BLOCK)
    dst = torch.zeros(rcx.encode_bound(n, BLOCK), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    things["encode"] = lambda: ctx.encode_blocks_device(src, BLOCK, dst, offs)
    things["decode"] = lambda: ctx.decode_blocks_device(dst, dst.numel(), offs, n, BLOCK, back)

    # warm-up and a check of what is measured: join(split(x)) = x for every width and predictor, decode(encode(x)) = x
    for width in WIDTHS:
        for name, pred in PREDS:
            for _ in range(2):
                things[f"split_{name}_w{width}"]()
                things[f"join_{name}_w{width}"]()
            ctx.sync_status()
            assert torch.equal(out, src), (width, name)
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

    rows = []
    yard = {k: stats(v, n) for k, v in kernels.items() if v}
    for width in WIDTHS:
        plain = {what: stats(ms[f"{what}_plain_w{width}"], n) for what in ("split", "join")}
        rows.append({"part": "plain", "kernel": "rcx_planes_k", "bytes": n, "block": BLOCK, "width": width, "data": "uniform mt19937(12345)", **plain,
                     "split_over_scatter": round(plain["split"]["ms_median"] / yard["scatter"]["ms_median"], 3),
                     "join_over_scatter": round(plain["join"]["ms_median"] / yard["scatter"]["ms_median"], 3)})
        for name, _ in PREDS[1:]:
            row = {"part": "fused", "kernel": "rcx_planes_k<W, false, PRED> / rcx_predict_join_k", "predictor": name, "bytes": n, "block": BLOCK, "width": width,
                   "data": "uniform mt19937(12345)"}
            for what, coder in (("split", "encode"), ("join", "decode")):
                s = row[what] = stats(ms[f"{what}_{name}_w{width}"], n)
                row[what + "_over_plain"] = round(s["ms_median"] / plain[what]["ms_median"], 3)
                row[f"{what}_share_of_{coder}"] = round(s["ms_median"] / yard[coder]["ms_median"], 4)
            spread = plain["split"]["ms_max"] - plain["split"]["ms_min"]
            med = row["split"]["ms_median"]
            row["split_outside_plain_spread"] = bool(med > plain["split"]["ms_max"] + spread or med < plain["split"]["ms_min"] - spread)
            rows.append(row)
    rows.append({"part": "yardsticks", "bytes": n, "block": BLOCK, "coder": "adaptive", "what": "the library's own event pairs around its kernels, same rounds",
                 "kernels": yard, "calls": {k: stats(ms[k], n) for k in ("encode", "decode")}})
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
