#!/usr/bin/env python3
"""Rates of rcx_typed_split_picks_device (include/rcx_typed_split_picks.h) next to the host-planned rcx_typed_items_split_device, by
the method of tools/typed_picks_rate.py: warm-up, 7 passes, everything that is compared alternated, median and min-max.  DESIGN.md
section 24 quotes profiles/r24_typed_split_picks_rate.jsonl.

    python tools/typed_split_picks_rate.py --baseline-library PATH [--out profiles/r24_typed_split_picks_rate.jsonl] [--repeats 7] [--parts A,B,C,D]

  A  200 000 items of 0 .. 4096 bytes, widths 2, 4, 8, all predictors, split.  Wall time of a call (host clock from the call to
     the return of a device synchronise) and GPU time (device events around it), both calls.  Bar: the device-planned call's wall
     median is no more than the host-planned call's median plus that call's own min-max spread in this run.
  B  the GiB as superblocks of w x 64 KiB, widths 2, 4, 8, without a predictor and with delta.  The walking launch alone (the
     context's RCX_T_ENCODE events around it) against the host-planned split's kernel (the call timed behind queued device copies
     that cover its host plan), and the planner (RCX_T_SCAN) on its own line.  Bar per width and predictor: the walking median
     is no more than the host-planned kernel's median plus its min-max spread.
  C  max_pick = 200 000 with *d_count = 100, 1000, 10 000, 200 000 of A's entries: GPU time of the call.  Report only.
  D  container.pack_typed_items_device + PackedTypedItems.decode_into on 20 000 of A's items (adaptive coder), eager and as one
     graph replay, beside pack_typed_items + unpack_typed_items' device path on the same items (the host-planned chain: host
     plan, uploads, split, encode, download; host plan, uploads, decode, join).  That path runs this build's library -- the
     container module binds one librcx a process -- whose host-planned kernels tools/diag/kernel_diff.py shows unchanged from the
     parent.  Report only.

--baseline-library: a librcx.so of the parent commit: the host-planned side of parts A and B is that library, never this build.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import container, encode_picks, picks, predict, rcx, typed_items, typed_picks, workloads  # noqa: E402
from cpprcoder_amd import typed_split_picks as tsp  # noqa: E402
import typed_picks_rate  # noqa: E402
from typed_picks_rate import BLOCK, WIDTHS, Baseline, alternated, dev8, dev64, marks_missed, opened, spread  # noqa: E402,F401  (the method is that tool's)


class Ragged(typed_picks_rate.Ragged):
    """Part A's batch: that tool's 200 000 items and their split text by the host-planned call of this build."""

    def __init__(self, ctx, count=200_000):
        super().__init__(ctx, count)
        self.d_kept = torch.zeros(count, dtype=torch.int64, device="cuda")
        tsp.reserve(ctx, count, self.total)

    def device_planned(self):
        tsp.split_device(self.ctx, self.items, self.d_at, self.d_at, self.d_len, self.d_w, self.d_p, self.d_count, self.out, self.total, kept=self.d_kept)

    def check(self, upto=None):
        self.ctx.sync_status()
        n = self.total if upto is None else int(self.offs[upto])
        assert torch.equal(self.out[:n], self.split[:n]), "the split entries are not the host-planned call's"


def part_a(w, args, emit, base):
    t = alternated({"device_planned": w.device_planned, "host_planned": lambda: base.split(w.items, w.offs, w.widths, w.preds, w.out)}, args.repeats)
    w.check()
    row = {"part": "A", "items": w.count, "bytes": w.total, "host_planned_by": "the parent commit's library"}
    for k, v in t.items():
        row[k] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    host = row["host_planned"]["wall_ms"]
    row["bar_ms"] = round(host["median"] + host["max"] - host["min"], 4)
    row["pass"] = row["device_planned"]["wall_ms"]["median"] <= row["bar_ms"]
    row["pass_mark"] = "device-planned call wall median <= host-planned call median + the host-planned min-max spread of this run"
    emit(row)


def part_b(ctx, args, emit, base):
    n = 1 << 30
    src, want, out, busy_a, busy_b = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(5))
    src.copy_(torch.from_numpy(workloads.uniform(n, 12345)).cuda())
    ctx.set_timing(True)
    for w in WIDTHS:
        sb = w * BLOCK
        lengths = np.array([sb] * (n // sb) + ([n % sb] if n % sb else []), np.uint64)
        offs, widths = rcx.item_offsets(lengths), np.full(len(lengths), w, np.uint8)
        d_at, d_len, d_w, d_count = dev64(offs[:-1]), dev64(lengths), dev8(widths), dev64([len(lengths)])
        tsp.reserve(ctx, len(lengths), n)
        for name, pred in (("none", predict.NONE), ("delta", predict.DELTA)):
            preds = np.full(len(lengths), pred, np.uint8)
            d_p = dev8(preds)
            typed_items.split_device(ctx, src, offs, widths, preds, want)
            ctx.sync_status()
            ctx.get_timing(reset=True)

            def cover(k):  # queued copies in front of the host-planned call: its kernel waits behind them while the host plans
                if k == "host_planned":
                    for _ in range(4):
                        busy_b.copy_(busy_a)

            fns = {"device_planned": lambda: tsp.split_device(ctx, src, d_at, d_at, d_len, d_w, d_p if pred else None, d_count, out, n),
                   "host_planned": lambda: base.split(src, offs, widths, preds, out)}
            t = alternated(fns, args.repeats, before=cover, after=lambda k: {s: v["ms"] for s, v in ctx.get_timing(reset=True).items() if s in ("scan", "encode")})
            ctx.sync_status()
            assert torch.equal(out, want), (w, name)
            walk = spread([a["encode"] for a in t["device_planned"]["after"]])
            planner = spread([a["scan"] for a in t["device_planned"]["after"]])
            host = spread(t["host_planned"]["gpu_ms"])
            bar = host["median"] + host["max"] - host["min"]
            emit({"part": "B", "width": w, "predictor": name, "items": len(lengths), "bytes": n,
                  "split_kernel_ms": {"device_planned_walk": walk, "host_planned_kernel_behind_copies": host}, "planner_ms": planner,
                  "device_planned_call_gpu_ms": spread(t["device_planned"]["gpu_ms"]), "walk_gbps": round(n / walk["median"] / 1e6, 1),
                  "bar_ms": round(bar, 4), "pass": walk["median"] <= bar,
                  "pass_mark": "walking launch's median <= host-planned split kernel's median + its min-max spread of this run",
                  "note": "the host-planned figure is device events around the call behind 4 queued GiB copies, so it holds the copies' tail and the upload"})
    ctx.set_timing(False)


def part_c(w, args, emit):
    row = {"part": "C", "max_pick": w.count, "what": "GPU time of one call (device events), the first `count` of part A's entries meant"}
    for count in (100, 1000, 10_000, w.count):
        w.d_count.fill_(count)
        w.out.zero_()
        t = alternated({"call": w.device_planned}, args.repeats)
        w.check(upto=count)
        row[f"count_{count}"] = {"gpu_ms": spread(t["call"]["gpu_ms"]), "wall_ms": spread(t["call"]["wall_ms"])}
    w.d_count.fill_(w.count)
    emit(row)


def part_d(w, args, emit, count=20_000):
    ctx = w.ctx
    total = int(w.offs[count])
    names = (None, "delta", "zigzag")
    parts = [w.items[int(w.offs[i]): int(w.offs[i + 1])] for i in range(count)]  # device tensors: the host-planned chain uploads no item
    widths, predict_ = [int(x) for x in w.widths[:count]], [names[int(p)] for p in w.preds[:count]]
    S = tsp.SLOTS
    max_len = 4096
    tsp.reserve(ctx, S * count, total)
    encode_picks.reserve(ctx, S * count, max_len, total)
    picks.reserve(ctx, S * count, max_len)
    typed_picks.reserve(ctx, S * count, total)
    d_pick = torch.arange(count, dtype=torch.int64, device="cuda")
    d_count = dev64([count])
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")

    def device_chain():
        packed = container.pack_typed_items_device(ctx, w.items, w.d_at, w.d_len, w.d_w, w.d_p, d_count, count, max_len, total)
        packed.decode_into(d_pick, w.d_at, d_count, out, count)
        return packed

    packed = device_chain()
    blob = packed.to_bytes()
    theirs = container.pack_typed_items(parts, widths=widths, predict=predict_, ctx=ctx)
    assert blob == theirs, "the device-packed container is not the host-planned one"
    assert torch.equal(out, w.items[:total])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        device_chain()
    pick = np.arange(count)

    def host_chain():
        c = container.parse_typed_items(container.pack_typed_items(parts, widths=widths, predict=predict_, ctx=ctx))
        container._unpack_items_device(ctx, c, pick, False)

    t = alternated({"graph_replay": g.replay, "eager": device_chain, "pack_typed_items_and_unpack_device_path_this_build": host_chain}, args.repeats)
    ctx.sync_status()
    assert torch.equal(out, w.items[:total])
    row = {"part": "D", "items": count, "bytes": total, "container_bytes": len(blob), "coder": "adaptive",
           "note": "the host-planned chain (pack_typed_items with its download and header, parse, _unpack_items_device without the download) runs this "
                   "build's library: its kernels are the parent's (tools/diag/kernel_diff.py), one process holds one librcx"}
    for k, v in t.items():
        row[k] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    emit(row)


def main():
    args, emit, rows = opened("r24_typed_split_picks_rate.jsonl")
    base = Baseline(args.baseline_library, "rcx_typed_items_split_device")
    ctx = rcx.Context(0)
    if {"A", "C", "D"} & set(args.parts):
        w = Ragged(ctx)
        if "A" in args.parts:
            part_a(w, args, emit, base)
        if "C" in args.parts:
            part_c(w, args, emit)
        if "D" in args.parts:
            part_d(w, args, emit)
        del w
    if "B" in args.parts:
        part_b(ctx, args, emit, base)
    ctx.close()
    marks_missed(rows)


if __name__ == "__main__":
    main()
