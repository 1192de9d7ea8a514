#!/usr/bin/env python3
"""Rate of the typed item calls (csrc/rcx_typed_items.hpp) beside the calls a user had before them: device events in one
process, warm-up, >= 5 rounds that alternate between everything measured, median and min-max.  DESIGN.md section 15 quotes
profiles/r13_typed_items_rate.jsonl; never bench.py's `value`.

    python tools/typed_items_rate.py [--out profiles/r13_typed_items_rate.jsonl] [--repeats 5] [--bytes N] [--items N]

Two ways of timing a call that plans on the host and uploads its tables before it launches:
  call     an event pair around the call on an idle GPU: the host plan, the upload and the kernels
  kernels  the same pair behind enough queued device copies to cover the plan: the first event fires when the copies end, the
           upload and the kernels are already queued behind it -- the upload and the kernels alone
The existing calls (rcx_predict_split_device / _join_device) plan nothing, so for them the two agree; they are timed the
first way, as tools/predict_rate.py times them.

(A) The mt19937(12345) GiB cut into its superblocks of w * 64 KiB as typed items, widths 2, 4 and 8: split, join without
    a predictor, split and join with delta -- each beside rcx_planes_k / rcx_predict_join_k through the existing call on
    the same bytes.  `over` = the item kernels' median over the existing call's.
(B) A ragged batch: 200 000 items of 0 to 4096 bytes, widths 2, 4, 8 and all three predictors mixed.  The call and the
    kernels alone, split and join; beside a loop of rcx_predict_split_device over the first 2 000 items, one call an item with
    its own width, predictor and a block of its element count + 1 -- what a user could do before.  Per-item costs, and
    whether their min-max ranges are apart.
Nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import predict, rcx, typed_items, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCK = 65536
WIDTHS = (2, 4, 8)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "repeats": len(ms)}
    if nbytes:
        out["ms_per_GiB"] = round(med * GIB / nbytes, 4)
        out["GBps_moved_median"] = round(2 * nbytes / 1e6 / med, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_typed_items_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--items", type=int, default=200_000)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    src, mid, out, busy_a, busy_b = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(5))
    assert all(r.data_ptr() % 16 == 0 for r in (src, mid, out))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())

    def behind(fn, copies):
        """fn timed behind `copies` queued device copies of the whole buffer (about half a millisecond a GiB each)."""
        def timed():
            for _ in range(copies):
                busy_b.copy_(busy_a)
            return once(fn)
        return timed

    # ---- (A) ------------------------------------------------------------------------------------------------------------
    things, tables = {}, {}
    for w in WIDTHS:
        sb = w * BLOCK
        lengths = np.array([sb] * (n // sb) + ([n % sb] if n % sb else []), np.uint64)
        offs, widths = rcx.item_offsets(lengths), np.full(len(lengths), w, np.uint8)
        tables[w] = (offs, widths)
        for name, pred in (("none", predict.NONE), ("delta", predict.DELTA)):
            preds = np.full(len(lengths), pred, np.uint8)
            things[f"block_split_{name}_w{w}"] = lambda w=w, pred=pred: once(lambda: predict.split_device(ctx, src, w, BLOCK, pred, mid))
            split = lambda offs=offs, widths=widths, preds=preds: typed_items.split_device(ctx, src, offs, widths, preds, mid)  # noqa: E731
            things[f"items_split_{name}_w{w}_call"] = lambda split=split: once(split)
            things[f"items_split_{name}_w{w}_kernels"] = behind(split, 4)
            things[f"block_join_{name}_w{w}"] = lambda w=w, pred=pred: once(lambda: predict.join_device(ctx, mid, w, BLOCK, pred, out))
            join = lambda offs=offs, widths=widths, preds=preds: typed_items.join_device(ctx, mid, offs, widths, preds, out)  # noqa: E731
            things[f"items_join_{name}_w{w}_call"] = lambda join=join: once(join)
            things[f"items_join_{name}_w{w}_kernels"] = behind(join, 4)
    # warm-up and a check of what is measured: the item calls write what the block calls write, and join(split(x)) = x
    check = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for w in WIDTHS:
        offs, widths = tables[w]
        for pred in (predict.NONE, predict.DELTA):
            preds = np.full(len(widths), pred, np.uint8)
            predict.split_device(ctx, src, w, BLOCK, pred, check)
            typed_items.split_device(ctx, src, offs, widths, preds, mid)
            typed_items.join_device(ctx, mid, offs, widths, preds, out)
            ctx.sync_status()
            assert torch.equal(mid, check) and torch.equal(out, src), (w, pred)
            out.zero_()
    del check
    ms = {k: [] for k in things}
    for _ in range(2):
        for fn in things.values():
            fn()
    for _ in range(args.repeats):  # one of each per round, in turn (a join always behind a split of the same width and predictor)
        for name, fn in things.items():
            ms[name].append(fn())
    rows = []
    for w in WIDTHS:
        for name in ("none", "delta"):
            row = {"part": "A", "bytes": n, "block": BLOCK, "width": w, "predictor": name, "items": len(tables[w][1]), "data": "uniform mt19937(12345)"}
            for what, yard in (("split", "rcx_planes_k"), ("join", "rcx_planes_k" if name == "none" else "rcx_predict_join_k")):
                blk = stats(ms[f"block_{what}_{name}_w{w}"], n)
                call, kern = stats(ms[f"items_{what}_{name}_w{w}_call"], n), stats(ms[f"items_{what}_{name}_w{w}_kernels"], n)
                row[what] = {"yardstick": yard, "block_call": blk, "items_call": call, "items_kernels": kern,
                             "kernels_over_block": round(kern["ms_median"] / blk["ms_median"], 3), "call_over_block": round(call["ms_median"] / blk["ms_median"], 3)}
            rows.append(row)

    # ---- (B) ------------------------------------------------------------------------------------------------------------
    rs = np.random.RandomState(13)
    count, first = args.items, 2000
    lengths = rs.randint(0, 4097, count).astype(np.uint64)
    widths = np.array(WIDTHS, np.uint8)[rs.randint(0, 3, count)]
    preds = rs.randint(0, 3, count).astype(np.uint8)
    offs = rcx.item_offsets(lengths)
    total = int(offs[-1])
    assert total <= n
    s, m, o = src[:total], mid[:total], out[:total]
    split = lambda: typed_items.split_device(ctx, s, offs, widths, preds, m)  # noqa: E731
    join = lambda: typed_items.join_device(ctx, m, offs, widths, preds, o)  # noqa: E731

    def loop():
        for i in range(first):
            a, b, w = int(offs[i]), int(offs[i + 1]), int(widths[i])
            if b > a:
                predict.split_device(ctx, src[a:b], w, max(16, (b - a) // w + 1), int(preds[i]), out[a:b])

    def host_plan():  # the call's host side alone: wall time of the enqueue, the GPU idle before and waited for after
        torch.cuda.synchronize()
        t = time.perf_counter()
        split()
        ms_ = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        return ms_

    split()
    join()
    ctx.sync_status()
    assert torch.equal(o, s)
    loop()
    ctx.sync_status()
    assert torch.equal(out[: int(offs[first])], m[: int(offs[first])])  # the loop writes what the call writes
    cover = 60  # queued copies in front of the kernels-alone timing: about 30 ms, more than the plan of 200 000 items takes
    things = {"split_call": lambda: once(split), "split_kernels": behind(split, cover), "join_call": lambda: once(join), "join_kernels": behind(join, cover),
              "split_enqueue_wall": host_plan, "loop_first_2000": lambda: once(loop)}
    ms = {k: [] for k in things}
    for fn in things.values():
        fn()
    for _ in range(args.repeats):
        for name, fn in things.items():
            ms[name].append(fn())
    per_item = {k: stats([v * 1e3 / (first if k.startswith("loop") else count) for v in ms[k]]) for k in ("split_call", "split_kernels", "loop_first_2000")}
    for v in per_item.values():
        v["unit"] = "microseconds an item"
    rows.append({"part": "B", "items": count, "bytes": total, "lengths": "0..4096 uniform, RandomState(13)", "widths": "2, 4, 8 mixed", "predictors": "none, delta, zigzag mixed",
                 **{k: stats(v, None if k in ("split_enqueue_wall", "loop_first_2000") else total) for k, v in ms.items()},
                 "loop_items": first, "loop_bytes": int(offs[first]), "per_item_us": per_item,
                 "call_below_loop_per_item": bool(per_item["split_call"]["ms_max"] < per_item["loop_first_2000"]["ms_min"]),
                 "loop_over_call_per_item": round(per_item["loop_first_2000"]["ms_median"] / per_item["split_call"]["ms_median"], 1)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
