#!/usr/bin/env python3
"""Rates of rcx_base_join_picks_device (include/rcx_base_picks.h) next to the host-planned rcx_base_items_join_device, by the
method of tools/typed_picks_rate.py: warm-up, 7 passes, everything that is compared alternated, median and min-max.  DESIGN.md
section 22 quotes profiles/r22_base_picks_rate.jsonl.

    python tools/base_picks_rate.py --baseline-library PATH [--out profiles/r22_base_picks_rate.jsonl] [--repeats 7] [--parts A,B,C,D]

  A  200 000 items of 0 .. 4096 bytes, widths 2, 4, 8, a third each without anything, with a predictor, with an op against a
     span of their own, all joined.  Wall time of a call (host clock from the call to the return of a device synchronise) and
     GPU time (device events around it), both calls.  Bar: the device-planned call's wall median is no more than the
     host-planned call's median plus that call's own min-max spread in this run.
  B  the GiB as superblocks of w x 64 KiB, widths 2, 4, 8, all with subzz against a second GiB.  The walking launches alone (the
     context's RCX_T_DECODE events around them) against the host-planned join's kernels (the call timed behind queued device
     copies that cover its host plan), and the planner (RCX_T_SCAN) on its own line.  Bar per width: the walking median is no
     more than the host-planned kernels' median plus their min-max spread.
  C  max_pick = 200 000 with *d_count = 100, 1000, 10 000, 200 000 of A's entries: GPU time of the call.  Report only.
  D  container.open_delta_items(...).decode_into on A's items packed as RCXK (adaptive coder), eager and as a graph replay,
     beside unpack_delta_items' device path for the same picks without the download (container._unpack_items_device: host plan,
     uploads, base check off, decode, join).  That path runs this build's library -- the container module binds one librcx a
     process -- whose host-planned kernels tools/diag/kernel_diff.py shows unchanged from the parent.  Bar by A's rule.

--baseline-library: a librcx.so of the PARENT commit: the host-planned side of parts A and B is that library, never this build,
loaded in a process of its own (this tool again with --serve, started once; it builds the same batches from the same seeds and
runs one pass a request, so the passes still alternate).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDTHS = (2, 4, 8)
BLOCK = 65536
NO_BASE = 0xFF
GIB = 1 << 30


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).cuda()


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint8))).cuda()


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "passes": len(ms)}


def noise(n, seed):
    """n bytes on the device, the same in both processes."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def ragged_tables(count=200_000):
    """Part A's batch -> (lengths, offsets, widths, preds, ops); an item with an op has its span at its own offset of the base."""
    rs = np.random.RandomState(13)
    lengths = rs.randint(0, 4097, count).astype(np.uint64)
    widths = np.array(WIDTHS, np.uint8)[rs.randint(0, 3, count)]
    kind = rs.randint(0, 9, count)  # 0 .. 2: nothing, 3 .. 5: a predictor, 6 .. 8: an op
    preds = np.where((kind >= 3) & (kind < 6), kind % 3 % 2 + 1, 0).astype(np.uint8)
    ops = np.where(kind >= 6, kind - 6, NO_BASE).astype(np.uint8)
    offs = np.zeros(count + 1, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    return lengths, offs, widths, preds, ops


def superblock_tables(w):
    sb = w * BLOCK
    lengths = np.array([sb] * (GIB // sb) + ([GIB % sb] if GIB % sb else []), np.uint64)
    offs = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(lengths, out=offs[1:])
    return lengths, offs, np.full(len(lengths), w, np.uint8), np.zeros(len(lengths), np.uint8), np.full(len(lengths), 2, np.uint8)


def timed(fn, before=None):
    """One pass -> (wall ms, GPU ms)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if before:
        before()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


# ---- the parent commit's library, in a process of its own ------------------------------------------------------------------------
class Library:
    """The host-planned calls of a build of the library (plain ctypes), on a context of its own."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
        self.L.rcx_ctx_create.argtypes = [i32, C.POINTER(vp)]
        for name in ("rcx_base_items_join_device", "rcx_base_items_split_device"):
            getattr(self.L, name).argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp]
        self.L.rcx_ctx_sync_status.argtypes = [vp, vp, vp]
        self.h = vp()
        assert self.L.rcx_ctx_create(0, C.byref(self.h)) == 0

    def call(self, name, src, ref, offs, boffs, widths, preds, ops, dst):
        st = getattr(self.L, name)(self.h, src.data_ptr(), ref.data_ptr(), offs.ctypes.data, boffs.ctypes.data, widths.ctypes.data, preds.ctypes.data,
                                   ops.ctypes.data, len(widths), dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, (name, st)

    def sync(self):
        assert self.L.rcx_ctx_sync_status(self.h, None, None) == 0


def serve(path):
    """Requests on stdin, one a line: `A` or `B <width>` prepares that batch (split by this library), `go` runs one pass of its
    join -- behind four queued GiB copies for B -- and answers `wall_ms gpu_ms`, `check` compares the output, `quit` ends."""
    lib = Library(path)
    state = {}
    for line in sys.stdin:
        words = line.split()
        if not words or words[0] == "quit":
            break
        if words[0] in ("A", "B"):
            state.clear()
            torch.cuda.empty_cache()
            lengths, offs, widths, preds, ops = ragged_tables() if words[0] == "A" else superblock_tables(int(words[1]))
            n = int(offs[-1])
            items, ref = noise(n, 12345), noise(n, 54321)
            mid, out = torch.zeros_like(items), torch.zeros_like(items)
            boffs = np.ascontiguousarray(offs[:-1])
            lib.call("rcx_base_items_split_device", items, ref, offs, boffs, widths, preds, ops, mid)
            lib.sync()
            busy = (torch.zeros(GIB, dtype=torch.uint8, device="cuda"), torch.zeros(GIB, dtype=torch.uint8, device="cuda")) if words[0] == "B" else None
            state.update(items=items, out=out, busy=busy, join=lambda: lib.call("rcx_base_items_join_device", mid, ref, offs, boffs, widths, preds, ops, out))
            print("ready", flush=True)
        elif words[0] == "go":
            def cover():
                if state["busy"]:
                    for _ in range(4):
                        state["busy"][1].copy_(state["busy"][0])
            wall, gpu = timed(state["join"], cover)
            print(f"{wall} {gpu}", flush=True)
        elif words[0] == "check":
            lib.sync()
            print("ok" if torch.equal(state["out"], state["items"]) else "differs", flush=True)


class Parent:
    """The serving process."""

    def __init__(self, path):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", path], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        answer = self.p.stdout.readline().strip()
        if not answer:
            raise SystemExit(f"the serving process ended at `{line}`")
        return answer

    def prepare(self, what):
        assert self.ask(what) == "ready"

    def go(self):
        wall, gpu = self.ask("go").split()
        return float(wall), float(gpu)

    def check(self):
        assert self.ask("check") == "ok", "the parent library's join did not give the items back"

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.close()
        self.p.wait(timeout=60)


# ---- this build ---------------------------------------------------------------------------------------------------------------------
def alternated(fns, repeats, warmup=2, after=None):
    """name -> a function that runs one pass and returns (wall ms, GPU ms), measured in turn."""
    for _ in range(warmup):
        for k, fn in fns.items():
            fn()
            if after:
                after(k)
    out = {k: {"gpu_ms": [], "wall_ms": [], "after": []} for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            wall, gpu = fn()
            out[k]["wall_ms"].append(wall)
            out[k]["gpu_ms"].append(gpu)
            if after:
                out[k]["after"].append(after(k))
    return out


class Ragged:
    """Part A's batch, split once by this build's host-planned call."""

    def __init__(self, ctx, base_items, base_picks):
        self.lengths, self.offs, self.widths, self.preds, self.ops = ragged_tables()
        self.count, self.total, self.ctx, self.calls = len(self.lengths), int(self.offs[-1]), ctx, base_picks
        self.items, self.ref = noise(self.total, 12345), noise(self.total, 54321)
        self.split, self.out = torch.zeros_like(self.items), torch.zeros_like(self.items)
        base_items.split_device(ctx, self.items, self.ref, self.offs, self.offs[:-1], self.widths, self.preds, self.ops, self.split)
        ctx.sync_status()
        self.d_at, self.d_len = dev64(self.offs[:-1]), dev64(self.lengths)
        self.d_w, self.d_p, self.d_o, self.d_count = dev8(self.widths), dev8(self.preds), dev8(self.ops), dev64([self.count])
        base_picks.reserve(ctx, self.count, self.total)

    def device_planned(self):
        self.calls.join_device(self.ctx, self.split, self.ref, self.d_at, self.d_at, self.d_at, self.d_len, self.d_w, self.d_p, self.d_o, self.d_count, self.out,
                               self.total)

    def check(self, upto=None):
        self.ctx.sync_status()
        n = self.total if upto is None else int(self.offs[upto])
        assert torch.equal(self.out[:n], self.items[:n]), "the joined entries are not the items"


def barred(row, ours, theirs, mark):
    row["bar_ms"] = round(theirs["median"] + theirs["max"] - theirs["min"], 4)
    row["pass"] = ours["median"] <= row["bar_ms"]
    row["bar"] = "met" if row["pass"] else "missed"
    row["pass_mark"] = mark


def part_a(w, args, emit, parent):
    parent.prepare("A")
    t = alternated({"device_planned": lambda: timed(w.device_planned), "host_planned": parent.go}, args.repeats)
    w.check()
    parent.check()
    row = {"part": "A", "items": w.count, "bytes": w.total, "host_planned_by": "the parent commit's library, in a process of its own"}
    for k, v in t.items():
        row[k] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    barred(row, row["device_planned"]["wall_ms"], row["host_planned"]["wall_ms"],
           "device-planned call wall median <= host-planned call median + the host-planned min-max spread of this run")
    emit(row)


def part_b(ctx, args, emit, parent, base_items, base_picks):
    src, ref = noise(GIB, 12345), noise(GIB, 54321)
    mid, out = torch.zeros_like(src), torch.zeros_like(src)
    ctx.set_timing(True)
    for w in WIDTHS:
        lengths, offs, widths, preds, ops = superblock_tables(w)
        d_at, d_len, d_w, d_o, d_count = dev64(offs[:-1]), dev64(lengths), dev8(widths), dev8(ops), dev64([len(lengths)])
        base_picks.reserve(ctx, len(lengths), GIB)
        base_items.split_device(ctx, src, ref, offs, offs[:-1], widths, preds, ops, mid)
        ctx.sync_status()
        ctx.get_timing(reset=True)
        parent.prepare(f"B {w}")
        fns = {"device_planned": lambda: timed(lambda: base_picks.join_device(ctx, mid, ref, d_at, d_at, d_at, d_len, d_w, None, d_o, d_count, out, GIB)),
               "host_planned": parent.go}
        t = alternated(fns, args.repeats, after=lambda k: {s: v["ms"] for s, v in ctx.get_timing(reset=True).items() if s in ("scan", "decode")})
        ctx.sync_status()
        parent.check()
        assert torch.equal(out, src), w
        walk = spread([a["decode"] for a in t["device_planned"]["after"]])
        planner = spread([a["scan"] for a in t["device_planned"]["after"]])
        host = spread(t["host_planned"]["gpu_ms"])
        row = {"part": "B", "width": w, "op": "subzz", "items": len(lengths), "bytes": GIB,
               "join_kernels_ms": {"device_planned_walk": walk, "host_planned_kernels_behind_copies": host}, "planner_ms": planner,
               "device_planned_call_gpu_ms": spread(t["device_planned"]["gpu_ms"]), "walk_gbps": round(GIB / walk["median"] / 1e6, 1),
               "note": "the host-planned figure is device events around the parent library's call behind 4 queued GiB copies, so it holds the copies' tail and the upload"}
        barred(row, walk, host, "walking launches' median <= host-planned join kernels' median + their min-max spread of this run")
        emit(row)
    ctx.set_timing(False)


def part_c(w, args, emit):
    row = {"part": "C", "max_pick": w.count, "what": "GPU time of one call (device events), the first `count` of part A's entries meant"}
    for count in (100, 1000, 10_000, w.count):
        w.d_count.fill_(count)
        w.out.zero_()
        t = alternated({"call": lambda: timed(w.device_planned)}, args.repeats)
        w.check(upto=count)
        row[f"count_{count}"] = {"gpu_ms": spread(t["call"]["gpu_ms"]), "wall_ms": spread(t["call"]["wall_ms"])}
    w.d_count.fill_(w.count)
    emit(row)


def part_d(w, args, emit, container):
    ctx = w.ctx
    host, ref = w.items.cpu().numpy(), w.ref.cpu().numpy()
    items = [host[int(w.offs[i]): int(w.offs[i + 1])] for i in range(w.count)]
    bases = [ref[int(w.offs[i]): int(w.offs[i + 1])] if w.ops[i] != NO_BASE else None for i in range(w.count)]
    blob = container.pack_delta_items(items, bases, widths=[int(x) for x in w.widths], ops=[(("xor", "sub", "subzz")[int(o)] if o != NO_BASE else None) for o in w.ops],
                                      predict=[(None, "delta", "zigzag")[int(p)] for p in w.preds], ctx=ctx)
    rs = np.random.RandomState(14)
    pick = rs.permutation(w.count)
    plen = w.lengths[pick]
    doffs = np.zeros(w.count + 1, np.uint64)
    np.cumsum(plen, out=doffs[1:])
    box = container.open_delta_items(blob, bases, ctx=ctx)
    box.reserve(w.count, w.total)
    d_pick, d_at, d_count = dev64(pick), dev64(doffs[:-1]), dev64([w.count])
    out = torch.zeros(w.total, dtype=torch.uint8, device="cuda")
    eager = lambda: box.decode_into(d_pick, d_at, d_count, out)  # noqa: E731
    eager()
    ctx.sync_status()
    want = torch.cat([w.items[int(w.offs[i]): int(w.offs[i + 1])] for i in pick[:2000]])
    assert torch.equal(out[: want.numel()], want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eager()
    k = container.parse_delta_items(blob)
    refs = container._picked_bases(k, pick, lambda i: bases[i])
    d_refs = [torch.from_numpy(np.concatenate(refs)).cuda()]  # (on the device, back to back in the picks' order: no gather or upload of the bases inside the path)
    fns = {"graph_replay": lambda: timed(g.replay), "eager": lambda: timed(eager),
           "unpack_delta_items_device_path_this_build": lambda: timed(lambda: container._unpack_items_device(ctx, k["inner"], pick, False, (k, d_refs, lambda i: None)))}
    t = alternated(fns, args.repeats)
    ctx.sync_status()
    assert torch.equal(out[: want.numel()], want)
    row = {"part": "D", "items": w.count, "bytes": w.total, "container_bytes": len(blob), "coder": "adaptive",
           "note": "unpack_delta_items' device path (host plan, uploads, decode, join; bases on the device, no check, no download) runs this build's library: "
                   "its kernels are the parent's (tools/diag/kernel_diff.py), one process holds one librcx"}
    for name, v in t.items():
        row[name] = {"wall_ms": spread(v["wall_ms"]), "gpu_ms": spread(v["gpu_ms"])}
    barred(row, row["eager"]["wall_ms"], row["unpack_delta_items_device_path_this_build"]["wall_ms"],
           "decode_into (eager) wall median <= unpack_delta_items' device path median + its min-max spread of this run")
    emit(row)
    box.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_base_picks_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parts", default="A,B,C,D")
    ap.add_argument("--baseline-library", help="a librcx.so of the parent commit: the host-planned side")
    ap.add_argument("--serve", help="(the tool's own: serve the host-planned calls of this library on stdin)")
    args = ap.parse_args()
    if args.serve:
        return serve(args.serve)
    if not args.baseline_library:
        ap.error("--baseline-library is required")
    args.parts = args.parts.split(",")
    if args.repeats < 5:
        ap.error("at least 5 passes")
    from cpprcoder_amd import base_items, base_picks, container, rcx
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:  # (kept up to date: a run that is cut short leaves what it had)
            for r in rows:
                f.write(json.dumps(r) + "\n")

    parent = Parent(os.path.abspath(args.baseline_library))
    ctx = rcx.Context(0)
    try:
        if {"A", "C", "D"} & set(args.parts):
            w = Ragged(ctx, base_items, base_picks)
            if "A" in args.parts:
                part_a(w, args, emit, parent)
            if "C" in args.parts:
                part_c(w, args, emit)
            if "D" in args.parts:
                part_d(w, args, emit, container)
            del w
            torch.cuda.empty_cache()
        if "B" in args.parts:
            part_b(ctx, args, emit, parent, base_items, base_picks)
    finally:
        parent.close()
    ctx.close()
    failed = [r for r in rows if r.get("pass") is False]
    if failed:
        print(f"{len(failed)} pass mark(s) missed", file=sys.stderr)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
