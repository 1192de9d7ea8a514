#!/usr/bin/env python3
"""Rates of the item calls (include/rcx.h, "Item calls") next to the block calls: device events around the enqueued
call, warm-up, >= 5 repeats, median and min-max.  DESIGN.md section 9 quotes profiles/r05_items_rate.jsonl; never
bench.py's `value`.

    python tools/items_rate.py [--out profiles/r05_items_rate.jsonl] [--repeats 7] [--baseline-library PATH] [--parts A,B,C,H]

  A  equal, aligned: the mt19937(12345) GiB as 16384 items of 64 KiB, item calls against block calls on the same bytes,
     alternated.  Pass mark: the item calls' median rate is not below the lowest rate the block calls showed.
  B  misaligned outputs: the same items decoded to d_dst + 1, + 7, + 15.  t_fast / t_slow = rcx_decode_blocks_device into
     an aligned destination / into d_dst + 1 (the whole wave symbol by symbol), measured in the same process through
     --baseline-library (a build of the commit before the item calls; without it, this build's own block calls).
     Pass mark: every item time below (t_fast + t_slow) / 2.
  C  ragged: lengths log-uniform over 4 KiB .. 256 KiB summing to 1 GiB of Zipf bytes, starts unaligned; work order on and
     off (RCX_ITEMS_ORDER=0), beside the block calls at 64 KiB (same bytes) and 256 KiB (same longest chain); all four
     coders, encode and decode.  Recorded, no pass mark.
  H  host time of one rcx_encode_items_device call for 200 000 items of 64 bytes (planning + table upload + launches;
     the call does not wait for the device), and of the planner alone.
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

from cpprcoder_amd import rcx, workloads  # noqa: E402

CODER_NAMES = ("adaptive", "static", "rans", "rans8")


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


def alternated(fns, repeats, warmup=2):
    """Several calls measured in turn, so that drift hits all of them alike -> {name: [ms]}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k] += timed(fn, 1, warmup=0)
    return out


def stats(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "MBps_median": round(nbytes / 1e3 / med, 1),
            "MBps_min": round(nbytes / 1e3 / max(ms), 1), "MBps_max": round(nbytes / 1e3 / min(ms), 1), "repeats": len(ms)}


class Baseline:
    """The block calls of another build of the library (plain ctypes: it need not know the item calls)."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        self.L.rcx_ctx_create.argtypes = [i32, C.POINTER(vp)]
        self.L.rcx_decode_blocks_device.argtypes = [vp, i32, vp, u64, vp, u64, u32, u64, vp, vp]
        self.L.rcx_ctx_sync_status.argtypes = [vp, vp, C.POINTER(u64)]
        self.L.rcx_ctx_destroy.argtypes = [vp]
        self.h = vp()
        assert self.L.rcx_ctx_create(0, C.byref(self.h)) == 0

    def decode_blocks_device(self, comp, comp_size, offs, n, block, out_ptr, coder):
        st = self.L.rcx_decode_blocks_device(self.h, coder, comp.data_ptr(), comp_size, offs.data_ptr(), rcx.block_count(n, block), block, n, out_ptr,
                                             torch.cuda.current_stream().cuda_stream)
        assert st == 0

    def sync(self):
        assert self.L.rcx_ctx_sync_status(self.h, torch.cuda.current_stream().cuda_stream, None) == 0


def part_ab(args, emit):
    n, block, coder = 1 << 30, 65536, CODER_NAMES.index(args.coder)
    data = workloads.uniform(n, 12345)
    ctx = rcx.Context(0)
    src = torch.from_numpy(data).cuda()
    nb = rcx.block_count(n, block)
    soffs = np.arange(nb + 1, dtype=np.uint64) * np.uint64(block)
    dst = torch.zeros(rcx.encode_bound(n, block, coder) + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    dst_i = torch.zeros_like(dst)
    offs_i = torch.zeros_like(offs)
    out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    ctx.encode_blocks_device(src, block, dst, offs, coder=coder)
    ctx.encode_items_device(src, soffs, dst_i, offs_i, coder=coder)
    ctx.sync_status()
    total = int(offs[-1])
    assert torch.equal(offs, offs_i) and torch.equal(dst[:total], dst_i[:total])
    if "A" in args.parts:
        enc = alternated({"blocks": lambda: ctx.encode_blocks_device(src, block, dst, offs, coder=coder),
                          "items": lambda: ctx.encode_items_device(src, soffs, dst_i, offs_i, coder=coder)}, args.repeats)
        dec = alternated({"blocks": lambda: ctx.decode_blocks_device(dst, total, offs, n, block, out[:n], coder=coder),
                          "items": lambda: ctx.decode_items_device(dst, total, offs, soffs, out[:n], coder=coder)}, args.repeats)
        ctx.sync_status()
        assert torch.equal(out[:n], src)
        for what, t in (("encode", enc), ("decode", dec)):
            b, i = stats(t["blocks"], n), stats(t["items"], n)
            emit({"part": "A", "what": what, "coder": args.coder, "items": nb, "item_bytes": block, "blocks": b, "item_call": i,
                  "pass": i["MBps_median"] >= b["MBps_min"], "pass_mark": "item median MB/s >= lowest block-call MB/s of the session"})
    if "B" in args.parts and coder in (0,):
        base = Baseline(args.baseline_library) if args.baseline_library else None

        def blocks_to(shift):
            view = out[shift: shift + n]
            if base:
                return lambda: base.decode_blocks_device(dst, total, offs, n, block, view.data_ptr(), coder)
            return lambda: ctx.decode_blocks_device(dst, total, offs, n, block, view, coder=coder)

        fns = {"t_fast": blocks_to(0), "t_slow": blocks_to(1)}
        for k in (1, 7, 15):
            fns[f"items+{k}"] = (lambda k=k: ctx.decode_items_device(dst, total, offs, soffs, out[k: k + n], coder=coder))
        t = alternated(fns, args.repeats)
        ctx.sync_status()
        if base:
            base.sync()
        assert torch.equal(out[15: 15 + n], src)
        fast, slow = stats(t["t_fast"], n), stats(t["t_slow"], n)
        mid = (fast["ms_median"] + slow["ms_median"]) / 2
        row = {"part": "B", "coder": args.coder, "baseline": "library of the parent commit" if base else "this build's block calls",
               "t_fast": fast, "t_slow": slow, "midpoint_ms": round(mid, 4)}
        ok = True
        for k in (1, 7, 15):
            row[f"items+{k}"] = stats(t[f"items+{k}"], n)
            ok = ok and row[f"items+{k}"]["ms_median"] < mid
        row["pass"] = ok
        row["pass_mark"] = "item decode at misalignment 1, 7, 15 below (t_fast + t_slow) / 2"
        emit(row)
    ctx.close()


def part_c(args, emit):
    n = 1 << 30
    data = workloads.zipf(n, 12345)
    rs = np.random.RandomState(2025)
    lengths = []
    left = n
    while left > 0:
        k = min(int(np.exp(rs.uniform(np.log(4096), np.log(262144)))), left)
        lengths.append(k)
        left -= k
    soffs = rcx.item_offsets(lengths)
    src = torch.from_numpy(data).cuda()
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for coder, name in enumerate(CODER_NAMES):
        ctx = rcx.Context(0)
        dst = torch.zeros(max(rcx.encode_items_bound(soffs, coder), rcx.encode_bound(n, 65536, coder)), dtype=torch.uint8, device="cuda")
        ioffs = torch.zeros(len(soffs), dtype=torch.int64, device="cuda")
        row = {"part": "C", "coder": name, "items": len(lengths), "bytes": n, "longest": int(max(lengths)), "shortest": int(min(lengths))}
        for order in ("sorted", "caller"):
            if order == "caller":
                os.environ["RCX_ITEMS_ORDER"] = "0"
            try:
                enc = timed(lambda: ctx.encode_items_device(src, soffs, dst, ioffs, coder=coder), args.repeats)
                ctx.sync_status()
                total = int(ioffs[-1])
                dec = timed(lambda: ctx.decode_items_device(dst, total, ioffs, soffs, out, coder=coder), args.repeats)
                ctx.sync_status()
            finally:
                os.environ.pop("RCX_ITEMS_ORDER", None)
            assert torch.equal(out, src)
            row[f"items_{order}_encode"], row[f"items_{order}_decode"] = stats(enc, n), stats(dec, n)
        for block in (65536, 262144):
            boffs = torch.zeros(rcx.block_count(n, block) + 1, dtype=torch.int64, device="cuda")
            enc = timed(lambda: ctx.encode_blocks_device(src, block, dst, boffs, coder=coder), args.repeats)
            ctx.sync_status()
            total = int(boffs[-1])
            dec = timed(lambda: ctx.decode_blocks_device(dst, total, boffs, n, block, out, coder=coder), args.repeats)
            ctx.sync_status()
            row[f"blocks_{block >> 10}K_encode"], row[f"blocks_{block >> 10}K_decode"] = stats(enc, n), stats(dec, n)
        emit(row)
        ctx.close()
        del dst


def part_h(args, emit):
    nitems = 200_000
    soffs = rcx.item_offsets(np.full(nitems, 64))
    src = torch.from_numpy(workloads.zipf(int(soffs[-1]), 3)).cuda()
    ctx = rcx.Context(0)
    dst = torch.zeros(rcx.encode_items_bound(soffs), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nitems + 1, dtype=torch.int64, device="cuda")
    call, plan = [], []
    for i in range(args.repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.encode_items_device(src, soffs, dst, offs)
        t1 = time.perf_counter()
        rcx.items_plan(soffs)
        t2 = time.perf_counter()
        if i >= 2:
            call.append((t1 - t0) * 1e3)
            plan.append((t2 - t1) * 1e3)
    ctx.sync_status()
    emit({"part": "H", "items": nitems, "item_bytes": 64, "what": "host milliseconds of one rcx_encode_items_device call (it does not wait for the device)",
          "call_ms_median": round(statistics.median(call), 3), "call_ms_min": round(min(call), 3), "call_ms_max": round(max(call), 3),
          "plan_only_ms_median": round(statistics.median(plan), 3), "repeats": len(call)})
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_items_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--coder", default="adaptive", choices=CODER_NAMES, help="parts A and B")
    ap.add_argument("--baseline-library", default=None, help="part B: librcx.so of the commit before the item calls")
    ap.add_argument("--parts", default="A,B,C,H")
    args = ap.parse_args()
    args.parts = args.parts.split(",")
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "A" in args.parts or "B" in args.parts:
        part_ab(args, emit)
    if "C" in args.parts:
        part_c(args, emit)
    if "H" in args.parts:
        part_h(args, emit)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    failed = [r for r in rows if r.get("pass") is False]
    if failed:
        print(f"{len(failed)} pass mark(s) missed", file=sys.stderr)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
