#!/usr/bin/env python3
"""Rates of rcx_encode_picks_device (include/rcx_encode_picks.h) next to the host-planned rcx_encode_items_device, by the method of
tools/picks_rate.py: warm-up, 7 passes, the two calls alternated, median and min-max.  DESIGN.md section 23 quotes
profiles/r23_encode_picks_rate.jsonl.

    python tools/encode_picks_rate.py --baseline-library PATH [--out profiles/r23_encode_picks_rate.jsonl] [--repeats 7] [--parts A,B,C,D]

The host-planned call is the PARENT commit's library's (--baseline-library: its librcx.so, loaded beside this build's with a
context of its own), never this tree's.

  A  200 000 items of 0 .. 4096 bytes of Zipf bytes, adaptive coder: wall time of a call (host clock from the call to the return
     of a device synchronise) and GPU time (device events around it), both calls.
  B  the ragged GiB of tools/items_rate.py part C (lengths log-uniform over 4 KiB .. 256 KiB), all four coders: the encode
     launches' time (each context's RCX_T_ENCODE events) of both calls, and what the device-planned call spends outside them (the
     planner, the size scan, the scatter).  Bar: the device-planned encode median is no more than the host-planned median plus the
     host-planned call's own min-max spread in this run.  A coder that misses it is recorded as missing it; nothing is raised.
  C  max_items = 200 000 with *d_count = 100, 1000, 10 000, 200 000 of A's items: device time of the call.  Live entries are not
     spread over the launch (not built): the rows say what a call costs as it is.
  D  A's workload: a captured graph's replay against the eager call, wall and GPU time.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import encode_picks as ep, rcx, workloads  # noqa: E402
from picks_rate import CODER_NAMES, alternated, dev64, opened, spread  # noqa: E402


class Baseline:
    """rcx_encode_items_device of another build of the library (plain ctypes), with a context and its timing events."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        self.L.rcx_ctx_create.argtypes = [i32, C.POINTER(vp)]
        self.L.rcx_encode_items_device.argtypes = [vp, i32, vp, vp, u64, vp, u64, vp, vp]
        self.L.rcx_ctx_sync_status.argtypes = [vp, vp, vp]
        self.L.rcx_ctx_set_timing.argtypes = [vp, i32]
        self.L.rcx_ctx_get_timing.argtypes = [vp, vp, vp, i32]
        self.L.rcx_ctx_destroy.argtypes = [vp]
        self.h = vp()
        assert self.L.rcx_ctx_create(0, C.byref(self.h)) == 0

    def encode_items_device(self, src, soffs, dst, offs, coder):
        st = self.L.rcx_encode_items_device(self.h, coder, src.data_ptr(), soffs.ctypes.data, len(soffs) - 1, dst.data_ptr(), dst.numel(), offs.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
        assert st == 0

    def sync(self):
        assert self.L.rcx_ctx_sync_status(self.h, None, None) == 0

    def set_timing(self, on):
        assert self.L.rcx_ctx_set_timing(self.h, int(on)) == 0

    def encode_ms(self):
        ms, launches = (C.c_double * rcx.T_COUNT)(), (C.c_uint64 * rcx.T_COUNT)()
        assert self.L.rcx_ctx_get_timing(self.h, ms, launches, 1) == 0
        return ms[0]

    def renew(self):
        """A fresh context: the scratch of the last workload is given back."""
        self.L.rcx_ctx_destroy(self.h)
        assert self.L.rcx_ctx_create(0, C.byref(self.h)) == 0


class SmallItems:
    """Part A's workload: 200 000 items of 0 .. 4096 bytes back to back, all meant."""

    def __init__(self, base, nitems=200_000, coder=0):
        rs = np.random.RandomState(2026)
        self.lengths = rs.randint(0, 4097, nitems).astype(np.uint64)
        self.soffs = rcx.item_offsets(self.lengths)
        self.n = int(self.soffs[-1])
        self.ctx, self.base, self.coder, self.nitems = rcx.Context(0), base, coder, nitems
        self.src = torch.from_numpy(workloads.zipf(self.n, 12345)).cuda()
        cap = max(rcx.encode_items_bound(self.soffs, coder), ep.dst_bound(nitems, self.n, coder))
        self.mine, self.theirs = (torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.my_offs, self.their_offs = (torch.zeros(nitems + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        self.d_at, self.d_len, self.d_count = dev64(self.soffs[:-1]), dev64(self.lengths), dev64([nitems])
        ep.reserve(self.ctx, nitems, 4096, self.n, coder)

    def device_planned(self):
        ep.encode_device(self.ctx, self.src, self.d_at, self.d_len, self.d_count, self.mine, self.my_offs, 4096, self.n, coder=self.coder)

    def host_planned(self):
        self.base.encode_items_device(self.src, self.soffs, self.theirs, self.their_offs, self.coder)

    def check(self, count=None):
        self.ctx.sync_status()
        self.base.sync()
        count = self.nitems if count is None else count
        total = int(self.their_offs[count])
        assert torch.equal(self.my_offs[: count + 1], self.their_offs[: count + 1]) and torch.equal(self.mine[:total], self.theirs[:total]), "the streams differ"


def part_a(w, args, emit):
    t = alternated({"device_planned": w.device_planned, "host_planned": w.host_planned}, args.repeats)
    w.check()
    row = {"part": "A", "coder": CODER_NAMES[w.coder], "items": w.nitems, "bytes": w.n, "host_planned_by": "the parent commit's library"}
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
    nitems, max_len = len(lengths), int(lengths.max())
    src = torch.from_numpy(data).cuda()
    d_at, d_len, d_count = dev64(soffs[:-1]), dev64(lengths), dev64([nitems])
    for coder, name in enumerate(CODER_NAMES):
        ctx = rcx.Context(0)
        base.renew()
        cap = max(rcx.encode_items_bound(soffs, coder), ep.dst_bound(nitems, n, coder))
        mine, theirs = (torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
        my_offs, their_offs = (torch.zeros(nitems + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        ep.reserve(ctx, nitems, max_len, n, coder)
        ctx.set_timing(True)
        base.set_timing(True)
        fns = {"device_planned": lambda: ep.encode_device(ctx, src, d_at, d_len, d_count, mine, my_offs, max_len, n, coder=coder),
               "host_planned": lambda: base.encode_items_device(src, soffs, theirs, their_offs, coder)}
        t = alternated(fns, args.repeats, after=lambda k: ctx.get_timing(reset=True)["encode"]["ms"] if k == "device_planned" else base.encode_ms())
        ctx.set_timing(False)
        base.set_timing(False)
        ctx.sync_status()
        base.sync()
        total = int(their_offs[-1])
        assert torch.equal(my_offs, their_offs) and torch.equal(mine[:total], theirs[:total]), "the streams differ"
        dev, host = spread(t["device_planned"]["after"]), spread(t["host_planned"]["after"])
        rest = [g - d for g, d in zip(t["device_planned"]["gpu_ms"], t["device_planned"]["after"])]
        bar = host["median"] + (host["max"] - host["min"])
        emit({"part": "B", "coder": name, "items": nitems, "bytes": n, "longest": max_len, "host_planned_by": "the parent commit's library",
              "encode_kernels_ms": {"device_planned": dev, "host_planned": host},
              "call_gpu_ms": {k: spread(v["gpu_ms"]) for k, v in t.items()}, "call_wall_ms": {k: spread(v["wall_ms"]) for k, v in t.items()},
              "bar_ms": round(bar, 4), "pass": dev["median"] <= bar,
              "pass_mark": "device-planned encode median <= host-planned median + the host-planned min-max spread of this run",
              "scratch_bytes": {"device_planned": ctx.scratch_bytes()}})
        emit({"part": "B", "coder": name, "what": "the device-planned call's GPU time less its encode launches: planner, size scan, scatter", "rest_ms": spread(rest)})
        ctx.close()
        del mine, theirs


def part_c(w, args, emit):
    row = {"part": "C", "coder": CODER_NAMES[w.coder], "max_items": w.nitems, "spread_live_entries": "not built",
           "what": "GPU time of one call (device events), the first `count` of part A's items meant"}
    for count in (100, 1000, 10_000, w.nitems):
        w.d_count.fill_(count)
        t = alternated({"call": w.device_planned}, args.repeats)
        w.check(count)
        row[f"count_{count}"] = {"gpu_ms": spread(t["call"]["gpu_ms"]), "wall_ms": spread(t["call"]["wall_ms"])}
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
    args, emit, rows = opened("r23_encode_picks_rate.jsonl")
    base = Baseline(args.baseline_library)
    if {"A", "C", "D"} & set(args.parts):
        w = SmallItems(base)
        w.host_planned()
        if "A" in args.parts:
            part_a(w, args, emit)
        if "C" in args.parts:
            part_c(w, args, emit)
        if "D" in args.parts:
            part_d(w, args, emit)
        w.ctx.close()
        del w
    if "B" in args.parts:
        part_b(args, emit, base)
    missed = [r["coder"] for r in rows if r.get("pass") is False]
    if missed:
        print(f"part B: the bar is missed by {', '.join(missed)} (recorded)", file=sys.stderr)


if __name__ == "__main__":
    main()
