#!/usr/bin/env python3
"""Rate of the fused candidate-cost call (csrc/rcx_typed_stats.hpp) beside the parent's way of getting the same table: device
events in one process, warm-up, >= 5 rounds that alternate between everything measured, median and min-max.  DESIGN.md
section 19 quotes profiles/r17_typed_stats_rate.jsonl; never bench.py's `value`.

    python tools/typed_stats_rate.py [--out profiles/r17_typed_stats_rate.jsonl] [--repeats 5] [--bytes N] [--items N]

A call that plans on the host and uploads its tables is timed as tools/base_items_rate.py times it: `call` is an event pair
around the call on an idle GPU, `kernels` the same pair behind enough queued device copies to cover the plan.

(A) The gate.  The mt19937(12345) GiB against the mt19937(54321) GiB cut into items of w * 64 KiB, widths 1, 2, 4, 8, k = 4 (none
    and the three ops) and, above width 1, k = 6.  The yardstick is the composition: for each asked candidate
    rcx_base_items_split_device and rcx_stats_items_device over the sub-items, 2 k calls, in the same rounds.  Required: the
    fused median below the composition's minimum (`fused_below_composition`), on the call and on the kernels alone.
(B) Skew, no gate: the GiB equal to its base, and a GiB of two alternating elements, beside the random GiB of (A); all
    candidates the width may ask for, the kernels alone.
(C) 200 000 items of 0 to 4096 bytes, widths and masks mixed: the call, the kernels alone, the enqueue's wall time.
(D) pack_tensors_delta of the GiB as eight uint16 tensors that moved a little, op="auto" beside op="subzz": wall time of the
    whole pack, download included.
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

from cpprcoder_amd import base_items, container, rcx, stats as stats_calls, typed_items, typed_stats as ts, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCK = 65536
WIDTHS = (1, 2, 4, 8)


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


def rounds(things, repeats):
    ms = {k: [] for k in things}
    for fn in things.values():
        fn()
    for _ in range(repeats):  # one of each per round, in turn
        for name, fn in things.items():
            ms[name].append(fn())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_typed_stats_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--items", type=int, default=200_000)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes
    ctx = rcx.Context(0)
    src, ref, mid, busy, other = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(5))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())
    ref.copy_(torch.from_numpy(workloads.uniform(n, 54321)).cuda())

    def behind(fn, copies):
        """fn timed behind `copies` queued device copies of the whole buffer (about half a millisecond a GiB each)."""
        def timed():
            for _ in range(copies):
                busy.copy_(other)
            return once(fn)
        return timed

    def cut(w):
        sb = w * BLOCK
        lengths = np.array([sb] * (n // sb) + ([n % sb] if n % sb else []), np.uint64)
        return rcx.item_offsets(lengths), np.full(len(lengths), w, np.uint8)

    rows = []
    # ---- (A) ------------------------------------------------------------------------------------------------------------
    things, shapes = {}, []
    for w in WIDTHS:
        offs, widths = cut(w)
        sub_offs = typed_items.sub_offsets(offs, widths)
        nitems, nsub = len(widths), len(sub_offs) - 1
        d_cost = torch.zeros(6 * nitems, dtype=torch.int64, device="cuda")
        d_sub = torch.zeros(6 * nsub, dtype=torch.int64, device="cuda")
        for mask in (ts.ALL_OPS,) + ((ts.ALL,) if w > 1 else ()):
            cands = [c for c in range(6) if mask >> c & 1]
            masks = np.full(nitems, mask, np.uint8)

            def fused(offs=offs, widths=widths, masks=masks, d_cost=d_cost):
                ts.items_device(ctx, src, ref, offs, offs[:-1], widths, masks, d_cost)

            def composed(offs=offs, widths=widths, sub_offs=sub_offs, cands=cands, d_sub=d_sub, nitems=nitems, nsub=nsub):
                for c in cands:
                    preds = np.full(nitems, c, np.uint8) if c in (1, 2) else None
                    ops = np.full(nitems, c - 3, np.uint8) if c >= 3 else None
                    base_items.split_device(ctx, src, ref, offs, offs[:-1], widths, preds, ops, mid)
                    stats_calls.items_device(ctx, mid, sub_offs, None, d_sub[c * nsub: (c + 1) * nsub])

            # what is measured is the same table: the composition's sub-item costs summed per item
            fused()
            composed()
            ctx.sync_status()
            sums = d_sub.view(6, nitems, w).sum(dim=2).t()
            got = d_cost.view(nitems, 6)
            assert all(torch.equal(got[:, c], sums[:, c]) for c in cands), (w, mask)
            k = len(cands)
            cover = 4 + 2 * k * (1 + nitems // 4096)
            key = f"w{w}_k{k}"
            shapes.append((key, w, k, nitems, mask))
            things[f"{key}_fused_call"] = lambda fused=fused: once(fused)
            things[f"{key}_fused_kernels"] = behind(fused, 4 + nitems // 4096)
            things[f"{key}_composed_call"] = lambda composed=composed: once(composed)
            things[f"{key}_composed_kernels"] = behind(composed, cover)
    ms = rounds(things, args.repeats)
    for key, w, k, nitems, mask in shapes:
        row = {"part": "A", "bytes": n, "block": BLOCK, "width": w, "k": k, "mask": mask, "items": nitems,
               "data": "uniform mt19937(12345) against uniform mt19937(54321)", "yardstick": "k x (rcx_base_items_split_device + rcx_stats_items_device)"}
        for how in ("call", "kernels"):
            f, c = stats(ms[f"{key}_fused_{how}"], n), stats(ms[f"{key}_composed_{how}"], n)
            row[how] = {"fused": f, "composed": c, "composed_over_fused": round(c["ms_median"] / f["ms_median"], 2),
                        "fused_below_composition": bool(f["ms_median"] < c["ms_min"] and f["ms_max"] < c["ms_min"])}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (B) ------------------------------------------------------------------------------------------------------------
    things = {}
    for w in WIDTHS:
        offs, widths = cut(w)
        masks = np.full(len(widths), ts.ALL if w > 1 else ts.ALL_OPS, np.uint8)
        d_cost = torch.zeros(6 * len(widths), dtype=torch.int64, device="cuda")
        two = torch.from_numpy(workloads.uniform(2 * w, 7)).cuda()
        alt = two.view(2, w).repeat(n // (2 * w), 1).reshape(-1)
        if alt.numel() < n:
            alt = torch.cat([alt, torch.zeros(n - alt.numel(), dtype=torch.uint8, device="cuda")])
        for name, a, b in (("random", src, ref), ("equal", ref, ref), ("alternating", alt, ref)):
            things[f"w{w}_{name}"] = behind(lambda a=a, b=b, offs=offs, widths=widths, masks=masks, d_cost=d_cost:
                                            ts.items_device(ctx, a, b, offs, offs[:-1], widths, masks, d_cost), 4 + len(widths) // 4096)
    ms = rounds(things, args.repeats)
    for w in WIDTHS:
        r = stats(ms[f"w{w}_random"], n)
        row = {"part": "B", "bytes": n, "width": w, "k": 6 if w > 1 else 4, "random": r}
        for name in ("equal", "alternating"):
            row[name] = stats(ms[f"w{w}_{name}"], n)
            row[f"{name}_over_random"] = round(row[name]["ms_median"] / r["ms_median"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (C) ------------------------------------------------------------------------------------------------------------
    rs = np.random.RandomState(17)
    count = args.items
    lengths = rs.randint(0, 4097, count).astype(np.uint64)
    widths = np.array(WIDTHS, np.uint8)[rs.randint(0, 4, count)]
    masks = np.where(widths == 1, np.array([ts.ALL_OPS, ts.ALL_OPS, 1], np.uint8)[rs.randint(0, 3, count)],
                     np.array([ts.ALL_OPS, ts.ALL, ts.ALL_PREDS], np.uint8)[rs.randint(0, 3, count)]).astype(np.uint8)
    offs = rcx.item_offsets(lengths)
    boffs = rcx.item_offsets(np.where(masks & ts.OP_BITS, lengths, 0).astype(np.uint64))
    total = int(offs[-1])
    assert total <= n
    d_cost = torch.zeros(6 * count, dtype=torch.int64, device="cuda")
    call = lambda: ts.items_device(ctx, src[:total], ref, offs, boffs[:-1], widths, masks, d_cost)  # noqa: E731

    def enqueue_wall():
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        ms_ = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        return ms_

    ms = rounds({"call": lambda: once(call), "kernels": behind(call, 80), "enqueue_wall": enqueue_wall}, args.repeats)
    rows.append({"part": "C", "items": count, "bytes": total, "base_bytes": int(boffs[-1]), "lengths": "0..4096 uniform, RandomState(17)",
                 "masks": "none + ops, all six, none + predictors (width 1: none + ops, none) mixed",
                 **{k: stats(v, None if k == "enqueue_wall" else total) for k, v in ms.items()},
                 "gpu_share_of_call": round(statistics.median(ms["kernels"]) / statistics.median(ms["call"]), 3),
                 "kernels_us_per_item": round(statistics.median(ms["kernels"]) * 1e3 / count, 4)})
    print(json.dumps(rows[-1]), flush=True)

    # ---- (D) ------------------------------------------------------------------------------------------------------------
    parts = 8
    per = n // (2 * parts)
    was = ref[: 2 * per * parts].view(torch.int16).view(parts, per)
    moved = was + torch.randint(-2, 3, was.shape, dtype=torch.int16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(17))
    named = {f"t{i}": moved[i] for i in range(parts)}
    before = {f"t{i}": was[i] for i in range(parts)}

    def pack(op):
        def timed():
            torch.cuda.synchronize()
            t = time.perf_counter()
            blob = container.pack_tensors_delta(named, before, BLOCK, op, ctx=ctx)
            timed.size = len(blob)
            return (time.perf_counter() - t) * 1e3
        return timed

    things = {"auto": pack("auto"), "subzz": pack("subzz")}
    ms = rounds(things, args.repeats)
    decided = container.choose_tensors_delta(named, before, BLOCK, "auto", None, ctx)[0]
    rows.append({"part": "D", "bytes": 2 * per * parts, "tensors": parts, "dtype": "int16", "data": "mt19937(54321) moved by -2 .. 2 an element",
                 "auto": stats(ms["auto"], 2 * per * parts), "subzz": stats(ms["subzz"], 2 * per * parts), "decided": sorted(set(map(str, decided.values()))),
                 "container_bytes": {k: v.size for k, v in things.items()}, "auto_over_subzz": round(statistics.median(ms["auto"]) / statistics.median(ms["subzz"]), 3),
                 "unit": "wall ms of the whole pack, download included"})
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
