#!/usr/bin/env python3
"""Rate of the base item calls (csrc/rcx_base_items.hpp) beside the block call of the same transform: device events in one
process, warm-up, >= 5 rounds that alternate between everything measured, median and min-max.  DESIGN.md section 18 quotes
profiles/r16_base_items_rate.jsonl; never bench.py's `value`.

    python tools/base_items_rate.py [--out profiles/r16_base_items_rate.jsonl] [--repeats 5] [--bytes N] [--items N]

A call that plans on the host and uploads its tables is timed as tools/typed_items_rate.py times it: `call` is an event pair
around the call on an idle GPU, `kernels` the same pair behind enough queued device copies to cover the plan -- the upload
and the kernels alone.

(A) Common ground.  The mt19937(12345) GiB against the mt19937(54321) GiB, cut into items of w * 64 KiB and of w * 16 KiB, every
    width and op, split and join, base_offsets == src_offsets: rcx_base_items_k beside rcx_base_k (the parent's kernel,
    unchanged) on the same bytes in the same rounds.  `over` = the item kernels' median over the block call's.  The margin is
    what the same table mechanism costs the parent's own kernels: rcx_typed_items_k over rcx_planes_k on the same item tables
    in the same run (widths 2, 4, 8, no predictor; width 1 takes the width-2 figure), times (1 + the yardstick's own
    (max - min) / median).
(B) Many small items: 200 000 items of 0 to 4096 bytes, every width and op and the items without a base mixed, the base spans
    packed.  The call and the kernels alone, the host's share; beside a loop of rcx_base_split_device over the first 2 000
    items that have an op, one call an item.
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

from cpprcoder_amd import base, base_items, planes, rcx, typed_items, workloads  # noqa: E402

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


def stats(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "repeats": len(ms)}
    if nbytes:
        out["ms_per_GiB"] = round(med * GIB / nbytes, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_base_items_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--items", type=int, default=200_000)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    src, ref, mid, out, busy = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(5))
    assert all(r.data_ptr() % 16 == 0 for r in (src, ref, mid, out))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())
    ref.copy_(torch.from_numpy(workloads.uniform(n, 54321)).cuda())

    def behind(fn, copies):
        """fn timed behind `copies` queued device copies of the whole buffer (about half a millisecond a GiB each)."""
        def timed():
            for _ in range(copies):
                busy.copy_(out)
            return once(fn)
        return timed

    rows = []
    # ---- (A) ------------------------------------------------------------------------------------------------------------
    for block in BLOCKS:
        things, tables = {}, {}
        for w in base.WIDTHS:
            sb = w * block
            lengths = np.array([sb] * (n // sb) + ([n % sb] if n % sb else []), np.uint64)
            offs, widths = rcx.item_offsets(lengths), np.full(len(lengths), w, np.uint8)
            tables[w] = (offs, widths)
            cover = 2 + len(lengths) // 8192  # (a plan of 8192 items takes well under the half millisecond of a copy)
            if w > 1:  # the margin's pair: the parent's kernels with and without the tables
                things[f"planes_split_w{w}"] = lambda w=w: once(lambda: planes.split_device(ctx, src, w, block, mid))
                things[f"typed_split_w{w}"] = behind(lambda offs=offs, widths=widths: typed_items.split_device(ctx, src, offs, widths, None, mid), cover)
                things[f"planes_join_w{w}"] = lambda w=w: once(lambda: planes.join_device(ctx, mid, w, block, out))
                things[f"typed_join_w{w}"] = behind(lambda offs=offs, widths=widths: typed_items.join_device(ctx, mid, offs, widths, None, out), cover)
            for name, op in OPS:
                ops = np.full(len(lengths), op, np.uint8)
                things[f"block_split_{name}_w{w}"] = lambda w=w, op=op: once(lambda: base.split_device(ctx, src, ref, w, block, op, mid))
                split = lambda offs=offs, widths=widths, ops=ops: base_items.split_device(ctx, src, ref, offs, offs[:-1], widths, None, ops, mid)  # noqa: E731
                things[f"items_split_{name}_w{w}_call"] = lambda split=split: once(split)
                things[f"items_split_{name}_w{w}_kernels"] = behind(split, cover)
                things[f"block_join_{name}_w{w}"] = lambda w=w, op=op: once(lambda: base.join_device(ctx, mid, ref, w, block, op, out))
                join = lambda offs=offs, widths=widths, ops=ops: base_items.join_device(ctx, mid, ref, offs, offs[:-1], widths, None, ops, out)  # noqa: E731
                things[f"items_join_{name}_w{w}_call"] = lambda join=join: once(join)
                things[f"items_join_{name}_w{w}_kernels"] = behind(join, cover)
        # warm-up and a check of what is measured: the item calls write what the block calls write, and join(split(x)) = x
        check = torch.zeros(n, dtype=torch.uint8, device="cuda")
        for w in base.WIDTHS:
            offs, widths = tables[w]
            for name, op in OPS:
                ops = np.full(len(widths), op, np.uint8)
                base.split_device(ctx, src, ref, w, block, op, check)
                base_items.split_device(ctx, src, ref, offs, offs[:-1], widths, None, ops, mid)
                base_items.join_device(ctx, mid, ref, offs, offs[:-1], widths, None, ops, out)
                ctx.sync_status()
                assert torch.equal(mid, check) and torch.equal(out, src), (block, w, name)
                out.zero_()
        del check
        ms = {k: [] for k in things}
        for fn in things.values():
            fn()
        for _ in range(args.repeats):  # one of each per round, in turn (a join always behind a split of the same width and op)
            for name, fn in things.items():
                ms[name].append(fn())
        for w in base.WIDTHS:
            mw = max(w, 2)
            margin = {}
            for what in ("split", "join"):
                yard, typed = stats(ms[f"planes_{what}_w{mw}"]), stats(ms[f"typed_{what}_w{mw}"])
                margin[what] = {"planes": yard, "typed_items_kernels": typed, "typed_over_planes": round(typed["ms_median"] / yard["ms_median"], 3)}
            for name, _ in OPS:
                row = {"part": "A", "bytes": n, "block": block, "width": w, "op": name, "items": len(tables[w][1]),
                       "data": "uniform mt19937(12345) against uniform mt19937(54321)"}
                for what in ("split", "join"):
                    blk = stats(ms[f"block_{what}_{name}_w{w}"], n)
                    call, kern = stats(ms[f"items_{what}_{name}_w{w}_call"], n), stats(ms[f"items_{what}_{name}_w{w}_kernels"], n)
                    m = round(margin[what]["typed_over_planes"] * (1 + (blk["ms_max"] - blk["ms_min"]) / blk["ms_median"]), 3)
                    over = round(kern["ms_median"] / blk["ms_median"], 3)
                    row[what] = {"yardstick": "rcx_base_k", "block_call": blk, "items_call": call, "items_kernels": kern, "kernels_over_block": over,
                                 "call_over_block": round(call["ms_median"] / blk["ms_median"], 3), "margin": m, "margin_from_width": mw,
                                 "typed_over_planes": margin[what]["typed_over_planes"], "above_margin": bool(over > m)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            if w > 1:
                rows.append({"part": "A margin", "bytes": n, "block": block, "width": w, **margin})

    # ---- (B) ------------------------------------------------------------------------------------------------------------
    rs = np.random.RandomState(16)
    count, first = args.items, 2000
    lengths = rs.randint(0, 4097, count).astype(np.uint64)
    widths = np.array(base.WIDTHS, np.uint8)[rs.randint(0, 4, count)]
    ops = np.array([0, 1, 2, base_items.NO_BASE], np.uint8)[rs.randint(0, 4, count)]
    preds = np.where((ops == base_items.NO_BASE) & (widths > 1), rs.randint(0, 3, count), 0).astype(np.uint8)
    offs = rcx.item_offsets(lengths)
    boffs = rcx.item_offsets(np.where(ops != base_items.NO_BASE, lengths, 0).astype(np.uint64))
    total = int(offs[-1])
    assert total <= n
    s, m, o = src[:total], mid[:total], out[:total]
    split = lambda: base_items.split_device(ctx, s, ref, offs, boffs[:-1], widths, preds, ops, m)  # noqa: E731
    join = lambda: base_items.join_device(ctx, m, ref, offs, boffs[:-1], widths, preds, ops, o)  # noqa: E731
    looped = [i for i in range(count) if ops[i] != base_items.NO_BASE and lengths[i]][:first]

    def loop():
        for i in looped:
            a, b, w, at = int(offs[i]), int(offs[i + 1]), int(widths[i]), int(boffs[i])
            base.split_device(ctx, src[a:b], ref[at: at + b - a], w, max(16, (b - a) // w + 1), int(ops[i]), out[a:b])

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
    assert all(torch.equal(out[int(offs[i]): int(offs[i + 1])], m[int(offs[i]): int(offs[i + 1])]) for i in looped[:200])  # the loop writes what the call writes
    cover = 80  # queued copies in front of the kernels-alone timing: about 40 ms, more than the plan of 200 000 items takes
    things = {"split_call": lambda: once(split), "split_kernels": behind(split, cover), "join_call": lambda: once(join), "join_kernels": behind(join, cover),
              "split_enqueue_wall": host_plan, "loop_first_2000": lambda: once(loop)}
    ms = {k: [] for k in things}
    for fn in things.values():
        fn()
    for _ in range(args.repeats):
        for name, fn in things.items():
            ms[name].append(fn())
    per_item = {k: stats([v * 1e3 / (len(looped) if k.startswith("loop") else count) for v in ms[k]]) for k in ("split_call", "split_kernels", "loop_first_2000")}
    for v in per_item.values():
        v["unit"] = "microseconds an item"
    rows.append({"part": "B", "items": count, "bytes": total, "base_bytes": int(boffs[-1]), "lengths": "0..4096 uniform, RandomState(16)",
                 "kinds": "widths 1, 2, 4, 8 x (xor, sub, subzz, no base with none, delta or zigzag) mixed",
                 **{k: stats(v, None if k in ("split_enqueue_wall", "loop_first_2000") else total) for k, v in ms.items()},
                 "gpu_share_of_split_call": round(statistics.median(ms["split_kernels"]) / statistics.median(ms["split_call"]), 3),
                 "loop_items": len(looped), "per_item_us": per_item,
                 "call_below_loop_per_item": bool(per_item["split_call"]["ms_max"] < per_item["loop_first_2000"]["ms_min"]),
                 "loop_over_call_per_item": round(per_item["loop_first_2000"]["ms_median"] / per_item["split_call"]["ms_median"], 1)})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
