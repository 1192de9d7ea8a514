#!/usr/bin/env python3
"""Rate of the stored-block mix (csrc/rcx_stored.hpp) beside rcx_scatter_k over the same streams, and what decoding a typed
fp32 buffer costs with and without stored blocks: device events around the enqueued call, one process, warm-up, >= 5 rounds
that alternate between everything measured, median and min-max.  DESIGN.md section 14 quotes profiles/r12_stored_rate.jsonl;
never bench.py's `value`.

    python tools/stored_rate.py [--out profiles/r12_stored_rate.jsonl] [--repeats 5] [--bytes N]

Part "mix", blocks of 64 KiB, the adaptive coder, gain 0: per buffer -- the mt19937(12345) GiB (bench.py's), a GiB of Zipf
bytes (16 MiB of workloads.zipf, repeated), a GiB of fp32 randn * 0.02 (rounded from double) split at width 4 -- one encode
with the context's timing on, whose scatter time is rcx_scatter_k over these streams, and one mix of its output.  The mix
reads the table, then every byte of the mixed set once, and writes it once; the scatter reads and writes the coded bytes.
Part "decode", the fp32 GiB at 16 KiB and at 64 KiB blocks, three ways: rcx_decode_blocks_device on the unmixed streams,
rcx_stored_decode_device on the mixed set (all blocks picked), and rcx_stored_decode_device with no block stored, which is
the item call on the unmixed streams: the cost of the item geometry and of planning and sending its tables.  The event
pair is recorded around the whole call, so the host's planning counts where the device waits for it.
Every row is time per call in milliseconds and scaled to one GiB.  Nothing here is a pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpprcoder_amd import planes, rcx, stored, workloads  # noqa: E402

GIB = float(1 << 30)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_per_GiB": round(med * GIB / nbytes, 4), "repeats": len(ms)}


class Coded:
    """A buffer on the device, its adaptive streams at one block size and their mixed set at gain 0."""

    def __init__(self, ctx, src, block):
        self.ctx, self.src, self.block, self.n = ctx, src, block, src.numel()
        self.nb = rcx.block_count(self.n, block)
        self.comp = torch.empty(rcx.encode_bound(self.n, block), dtype=torch.uint8, device="cuda")
        self.offs = torch.zeros(self.nb + 1, dtype=torch.int64, device="cuda")
        self.mixed = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        self.moffs = torch.zeros(self.nb + 1, dtype=torch.int64, device="cuda")
        self.flags = torch.zeros(self.nb, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        self.scatter_ms = []
        self.encode()
        self.mix()
        ctx.sync_status()
        ctx.get_timing(reset=True)
        self.scatter_ms.clear()
        self.coded, self.mixed_size = int(self.offs[-1]), int(self.moffs[-1])
        self.host_flags = self.flags.cpu().numpy()
        self.doffs = np.minimum(np.arange(self.nb + 1, dtype=np.uint64) * np.uint64(block), np.uint64(self.n))

    def encode(self):
        self.ctx.encode_blocks_device(self.src, self.block, self.comp, self.offs)
        self.scatter_ms.append(self.ctx.get_timing(reset=True)["scatter"]["ms"])  # (waits for the events)

    def mix(self):
        stored.mix_device(self.ctx, self.src, self.block, self.comp, self.comp.numel(), self.offs, 0, self.mixed, self.moffs, self.flags)

    def decode_blocks(self):
        self.ctx.decode_blocks_device(self.comp, self.coded, self.offs, self.n, self.block, self.out)

    def decode_mixed(self):
        stored.decode_device(self.ctx, self.mixed, self.mixed_size, self.moffs, self.host_flags, self.doffs, self.out)

    def decode_items(self):
        stored.decode_device(self.ctx, self.comp, self.coded, self.offs, None, self.doffs, self.out)

    def check(self, what):
        self.ctx.sync_status()
        assert torch.equal(self.out, self.src), what
        self.out.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_stored_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes // (4 * 65536) * (4 * 65536)  # whole superblocks of fp32 at 64 KiB blocks
    ctx = rcx.Context(0)
    ctx.set_timing(True)

    piece = torch.from_numpy(workloads.zipf(min(n, 16 << 20), 12345)).cuda()
    values = (torch.randn(n // 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(12345)) * 0.02).to(torch.float32)
    d_values = values.view(torch.uint8)
    split = {block: torch.empty(n, dtype=torch.uint8, device="cuda") for block in (16384, 65536)}
    for block, d_split in split.items():
        planes.split_device(ctx, d_values, 4, block, d_split)
    data = {"uniform mt19937(12345)": torch.from_numpy(workloads.uniform(n, 12345)).cuda(),
            "zipf, 16 MiB repeated": piece.repeat(-(-n // piece.numel()))[:n].contiguous(),
            "fp32 randn * 0.02, split at width 4": split[65536]}
    mixes = {name: Coded(ctx, src, 65536) for name, src in data.items()}
    decodes = {65536: mixes["fp32 randn * 0.02, split at width 4"], 16384: Coded(ctx, split[16384], 16384)}

    things = {}
    for name, c in mixes.items():
        things[("mix", name, "encode")] = c.encode
        things[("mix", name, "mix")] = c.mix
    for block, c in decodes.items():
        for way in ("decode_blocks", "decode_mixed", "decode_items"):
            things[("decode", block, way)] = getattr(c, way)

    # warm-up and a check of what is measured: every decode gives the split text back, the mixed set is the mirror's on the first blocks
    for _ in range(2):
        for fn in things.values():
            fn()
    for block, c in decodes.items():
        for way in ("decode_blocks", "decode_mixed", "decode_items"):
            getattr(c, way)()
            c.check((block, way))
    for name, c in mixes.items():
        k = 8
        offs, moffs = c.offs[: k + 1].cpu().numpy().astype(np.uint64), c.moffs[: k + 1].cpu().numpy().astype(np.uint64)
        want = stored.mix_numpy(c.src[: k * 65536].cpu().numpy(), 65536, c.comp[: int(offs[-1])].cpu().numpy(), offs, 0)
        assert np.array_equal(want[1], moffs) and np.array_equal(want[0], c.mixed[: int(moffs[-1])].cpu().numpy()) and np.array_equal(want[2], c.host_flags[:k]), name
        c.scatter_ms.clear()

    ms = {k: [] for k in things}
    for _ in range(args.repeats):  # one of each per round, in turn
        for key, fn in things.items():
            ms[key].append(once(fn))
    ctx.sync_status()

    rows = []
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, c in mixes.items():
        scatter = statistics.median(c.scatter_ms)
        rows.append({"part": "mix", "bytes": n, "block": 65536, "coder": "adaptive", "gain": 0, "data": name, "coded_bytes": c.coded, "mixed_bytes": c.mixed_size,
                     "stored_blocks": int(c.host_flags.sum()), "blocks": c.nb, "mix": summary(ms[("mix", name, "mix")], n),
                     "scatter": summary(c.scatter_ms, n), "encode_call": summary(ms[("mix", name, "encode")], n),
                     "mix_over_scatter": round(med[("mix", name, "mix")] / scatter, 3)})
    for block, c in decodes.items():
        row = {"part": "decode", "bytes": n, "block": block, "coder": "adaptive", "gain": 0, "data": "fp32 randn * 0.02, split at width 4",
               "coded_bytes": c.coded, "mixed_bytes": c.mixed_size, "stored_blocks": int(c.host_flags.sum()), "blocks": c.nb}
        for way in ("decode_blocks", "decode_mixed", "decode_items"):
            row[way] = summary(ms[("decode", block, way)], n)
        row["mixed_over_blocks"] = round(med[("decode", block, "decode_mixed")] / med[("decode", block, "decode_blocks")], 3)
        row["items_over_blocks"] = round(med[("decode", block, "decode_items")] / med[("decode", block, "decode_blocks")], 3)
        rows.append(row)
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
