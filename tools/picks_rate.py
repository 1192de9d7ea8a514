#!/usr/bin/env python3
"""Rates of rcx_decode_picks_device (include/rcx_picks.h) next to the host-planned rcx_decode_items_device: warm-up, >= 5
passes, the two calls alternated, median and min-max.  DESIGN.md section 20 quotes profiles/r10_picks_rate.jsonl.

    python tools/picks_rate.py [--out profiles/r10_picks_rate.jsonl] [--repeats 7] [--parts A,B,C,D] [--baseline-library PATH]

  A  200 000 items of 0 .. 4096 bytes of Zipf bytes, all picked in a shuffled order: wall time of a call (host clock from
     the call to the return of a device synchronise) and GPU time (device events around it), both calls.
  B  the ragged GiB of tools/items_rate.py part C (lengths log-uniform over 4 KiB .. 256 KiB), all four coders: the decode
     launches' time (the context's RCX_T_DECODE events) of both calls, and the planner's time on its own line (the
     call's device time less its decode launches).  Bar: the device-planned decode median is no more than the host-planned
     median plus the host-planned call's own min-max spread in this run.
  C  max_pick = 200 000 with *d_count = 100, 1000, 10 000 of A's items: device time of the call.  Live entries are not spread
     over the launch (not built): the rows say what a call costs as it is.
  D  A's workload: a captured graph's replay against the eager call, wall and GPU time.

--baseline-library: a librcx.so of the parent commit for the host-planned call (tools/diag/kernel_diff.py shows its decode
kernels unchanged in this build, which is what is used without the option).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import picks, rcx, workloads  # noqa: E402

CODER_NAMES = ("adaptive", "static", "rans", "rans8")


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "passes": len(ms)}


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint8))).cuda()


def alternated(fns, repeats, warmup=2, after=None, before=None):
    """Several calls measured in turn -> {name: {"gpu_ms": [...], "wall_ms": [...], "after": [...]}}: device events around the
    call, and the host clock from the call to the return of a device synchronise; before(name) runs in front of the first
    event (what it enqueues is outside the events and keeps the device busy while the call's host side runs), after(name) is
    called behind each."""
    for _ in range(warmup):
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            if after:
                after(k)
    out = {k: {"gpu_ms": [], "wall_ms": [], "after": []} for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            if before:
                before(k)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            out[k]["gpu_ms"].append(a.elapsed_time(b))
            if after:
                out[k]["after"].append(after(k))
    return out


def opened(out_name, baseline_required=True):
    """The command line of a *_picks_rate tool -> (args, emit, rows): emit(row) prints the row and rewrites args.out with every
    row so far (a run that is cut short leaves what it had)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parts", default="A,B,C,D")
    ap.add_argument("--baseline-library", required=baseline_required, help="a librcx.so of the parent commit: the host-planned side")
    ap.add_argument("--build-note", default=None, help="goes into every row as `build`: which build of the library a run measured")
    args = ap.parse_args()
    args.parts = args.parts.split(",")
    if args.repeats < 5:
        ap.error("at least 5 passes")
    rows = []

    def emit(row):
        if args.build_note:
            row["build"] = args.build_note
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")

    return args, emit, rows


def marks_missed(rows):
    failed = [r for r in rows if r.get("pass") is False]
    if failed:
        print(f"{len(failed)} pass mark(s) missed", file=sys.stderr)
        raise SystemExit(1)


class Baseline:
    """rcx_decode_items_device of another build of the library (plain ctypes)."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        self.L.rcx_ctx_create.argtypes = [i32, C.POINTER(vp)]
        self.L.rcx_decode_items_device.argtypes = [vp, i32, vp, u64, vp, u64, vp, u64, vp, vp, vp]
        self.L.rcx_ctx_destroy.argtypes = [vp]
        self.h = vp()
        assert self.L.rcx_ctx_create(0, C.byref(self.h)) == 0

    def decode_items_device(self, comp, comp_size, offs, doffs, out, pick, coder):
        st = self.L.rcx_decode_items_device(self.h, coder, comp.data_ptr(), comp_size, offs.data_ptr(), offs.numel() - 1, pick.ctypes.data, len(pick),
                                            doffs.ctypes.data, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0


class SmallItems:
    """Part A's workload, encoded once: 200 000 items of 0 .. 4096 bytes, all picked in a shuffled order."""

    def __init__(self, nitems=200_000, coder=0):
        rs = np.random.RandomState(2026)
        self.lengths = rs.randint(0, 4097, nitems).astype(np.uint64)
        soffs = rcx.item_offsets(self.lengths)
        self.n = int(soffs[-1])
        self.ctx = rcx.Context(0)
        self.src = torch.from_numpy(workloads.zipf(self.n, 12345)).cuda()
        self.comp = torch.zeros(rcx.encode_items_bound(soffs, coder), dtype=torch.uint8, device="cuda")
        self.offs = torch.zeros(nitems + 1, dtype=torch.int64, device="cuda")
        self.ctx.encode_items_device(self.src, soffs, self.comp, self.offs, coder=coder)
        self.ctx.sync_status()
        self.total = int(self.offs[-1])
        self.pick = rs.permutation(nitems).astype(np.uint64)
        self.plen = self.lengths[self.pick.astype(np.int64)]
        self.doffs = rcx.item_offsets(self.plen)
        self.out = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        self.want = torch.cat([self.src[int(soffs[i]): int(soffs[i + 1])] for i in self.pick[:2000].astype(np.int64)])
        self.d_pick, self.d_at, self.d_len = dev64(self.pick), dev64(self.doffs[:-1]), dev64(self.plen)
        self.d_count = dev64([nitems])
        self.coder, self.nitems = coder, nitems
        picks.reserve(self.ctx, nitems, 4096, coder)

    def device_planned(self):
        picks.decode_device(self.ctx, self.comp, self.total, self.offs, self.d_pick, self.d_at, self.d_len, self.d_count, self.out, 4096, coder=self.coder)

    def host_planned(self, base=None):
        if base:
            base.decode_items_device(self.comp, self.total, self.offs, self.doffs, self.out, self.pick, self.coder)
        else:
            self.ctx.decode_items_device(self.comp, self.total, self.offs, self.doffs, self.out, pick=self.pick, coder=self.coder)

    def check(self):
        self.ctx.sync_status()
        assert torch.equal(self.out[: self.want.numel()], self.want), "the decoded picks are not the items"


def part_a(w, args, emit, base):
    t = alternated({"device_planned": w.device_planned, "host_planned": lambda: w.host_planned(base)}, args.repeats)
    w.check()
    row = {"part": "A", "coder": CODER_NAMES[w.coder], "items": w.nitems, "bytes": w.n, "host_planned_by": "the parent commit's library" if base else "this build"}
    for k, v in t.items():
        row[k] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    emit(row)


def part_b(args, emit, base):
    n = 1 << 30
    data = workloads.zipf(n, 12345)
    rs = np.random.RandomState(2025)
    lengths, left = [], n
    while left > 0:
        k = min(int(np.exp(rs.uniform(np.log(4096), np.log(262144)))), left)
        lengths.append(k)
        left -= k
    lengths = np.array(lengths, dtype=np.uint64)
    soffs = rcx.item_offsets(lengths)
    nitems = len(lengths)
    src = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_pick, d_at, d_len, d_count = dev64(np.arange(nitems)), dev64(soffs[:-1]), dev64(lengths), dev64([nitems])
    max_len = int(lengths.max())
    for coder, name in enumerate(CODER_NAMES):
        ctx = rcx.Context(0)
        comp = torch.zeros(rcx.encode_items_bound(soffs, coder), dtype=torch.uint8, device="cuda")
        offs = torch.zeros(nitems + 1, dtype=torch.int64, device="cuda")
        ctx.encode_items_device(src, soffs, comp, offs, coder=coder)
        ctx.sync_status()
        total = int(offs[-1])
        picks.reserve(ctx, nitems, max_len, coder)
        ctx.set_timing(True)
        ctx.get_timing(reset=True)
        fns = {"device_planned": lambda: picks.decode_device(ctx, comp, total, offs, d_pick, d_at, d_len, d_count, out, max_len, coder=coder),
               "host_planned": lambda: ctx.decode_items_device(comp, total, offs, soffs, out, coder=coder)}
        t = alternated(fns, args.repeats, after=lambda k: ctx.get_timing(reset=True)["decode"]["ms"])
        ctx.set_timing(False)
        ctx.sync_status()
        assert torch.equal(out, src)
        dev, host = spread(t["device_planned"]["after"]), spread(t["host_planned"]["after"])
        planner = [g - d for g, d in zip(t["device_planned"]["gpu_ms"], t["device_planned"]["after"])]
        bar = host["median"] + (host["max"] - host["min"])
        emit({"part": "B", "coder": name, "items": nitems, "bytes": n, "longest": max_len, "decode_kernels_ms": {"device_planned": dev, "host_planned": host},
              "call_gpu_ms": {k: spread(v["gpu_ms"]) for k, v in t.items()}, "call_wall_ms": {k: spread(v["wall_ms"]) for k, v in t.items()},
              "bar_ms": round(bar, 4), "pass": dev["median"] <= bar,
              "pass_mark": "device-planned decode median <= host-planned median + the host-planned min-max spread of this run"})
        emit({"part": "B", "coder": name, "what": "the planner: the device-planned call's GPU time less its decode launches", "planner_ms": spread(planner)})
        ctx.close()
        del comp


def part_c(w, args, emit):
    row = {"part": "C", "coder": CODER_NAMES[w.coder], "max_pick": w.nitems, "spread_live_entries": "not built",
           "what": "GPU time of one call (device events), the first `count` of part A's picks meant"}
    for count in (100, 1000, 10_000, w.nitems):
        w.d_count.fill_(count)
        t = alternated({"call": w.device_planned}, args.repeats)
        row[f"count_{count}"] = {"gpu_ms": spread(t["call"]["gpu_ms"]), "wall_ms": spread(t["call"]["wall_ms"])}
    w.ctx.sync_status()
    emit(row)


def part_d(w, args, emit):
    w.d_count.fill_(w.nitems)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.device_planned()
    t = alternated({"graph_replay": g.replay, "eager": w.device_planned}, args.repeats)
    w.check()
    row = {"part": "D", "coder": CODER_NAMES[w.coder], "items": w.nitems, "bytes": w.n}
    for k, v in t.items():
        row[k] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    emit(row)


def main():
    args, emit, rows = opened("r10_picks_rate.jsonl", baseline_required=False)
    base = Baseline(args.baseline_library) if args.baseline_library else None
    if {"A", "C", "D"} & set(args.parts):
        w = SmallItems()
        if "A" in args.parts:
            part_a(w, args, emit, base)
        if "C" in args.parts:
            part_c(w, args, emit)
        if "D" in args.parts:
            part_d(w, args, emit)
        w.ctx.close()
        del w
    if "B" in args.parts:
        part_b(args, emit, None)
    marks_missed(rows)


if __name__ == "__main__":
    main()
