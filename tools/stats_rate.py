#!/usr/bin/env python3
"""Rate of the block statistics kernel (csrc/rcx_stats.hpp) beside the CRC-32 kernel over the same bytes, and what
pack_typed(predict="auto") pays for its decision beside one encode: device events around the enqueued call, one process,
warm-up, >= 5 rounds that alternate between everything measured, median and min-max.  DESIGN.md section 13 quotes
profiles/r08_stats_rate.jsonl; never bench.py's `value`.

    python tools/stats_rate.py [--out profiles/r08_stats_rate.jsonl] [--repeats 5] [--bytes N]

Blocks of 64 KiB, costs only (d_hist null, as the decision calls it).  Per buffer -- the mt19937(12345) GiB (bench.py's),
a GiB of one repeated byte, a GiB of two alternating values, the split text of a GiB of sorted int64 keys under delta --
the kernel and rcx_crc32_k: both read n bytes and write next to nothing.  Then on the sorted keys the whole decision (three
splits, three statistics passes, one download of three sums) and one adaptive encode of the split text.  (The rows
`stats_plain` of the file on record are the kernel before equal neighbours were merged, taken in the same rounds by a
build that still carried both forms.)
Every row is time per call in milliseconds and scaled to one GiB; *_over_crc is the median over the CRC kernel's on the same
bytes, *_over_uniform over the same form's on the uniform GiB.  Nothing here is a pass mark.
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

from cpprcoder_amd import container, predict, rcx, stats, workloads  # noqa: E402

GIB = float(1 << 30)
BLOCK = 65536


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_per_GiB": round(med * GIB / nbytes, 4),
            "GBps_read_median": round(nbytes / 1e6 / med, 1), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_stats_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes // (8 * BLOCK) * (8 * BLOCK)  # whole superblocks of int64
    ctx = rcx.Context(0)
    nb = rcx.block_count(n, BLOCK)

    keys = torch.sort(torch.randint(0, 10 ** 9 * max(n >> 20, 1), (n // 8,), dtype=torch.int64, device="cuda", generator=torch.Generator("cuda").manual_seed(12345)))[0]
    d_keys = keys.view(torch.uint8)
    d_split = torch.empty(n, dtype=torch.uint8, device="cuda")
    data = {"uniform mt19937(12345)": torch.from_numpy(workloads.uniform(n, 12345)).cuda(),
            "one repeated byte": torch.full((n,), 0xA7, dtype=torch.uint8, device="cuda"),
            "two alternating values": torch.tensor([0x00, 0xFF], dtype=torch.uint8, device="cuda").repeat(n // 2),
            "sorted int64 keys, delta, split": torch.empty(n, dtype=torch.uint8, device="cuda")}
    predict.split_device(ctx, d_keys, 8, BLOCK, predict.DELTA, data["sorted int64 keys, delta, split"])
    d_cost = torch.zeros(nb, dtype=torch.int64, device="cuda")
    d_crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
    dst = torch.zeros(rcx.encode_bound(n, BLOCK), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")

    things = {}
    for name, src in data.items():
        things[(name, "stats_merged")] = lambda src=src: stats.blocks_device(ctx, src, BLOCK, None, d_cost)
        things[(name, "crc32")] = lambda src=src: ctx.crc32_blocks_device(src, BLOCK, d_crc)
    choice = []

    def decide():
        choice.append(container._measured_predictor(ctx, d_keys, 8, BLOCK, nb, d_split)[0])

    things[("sorted int64 keys", "auto_decision")] = decide
    things[("sorted int64 keys", "encode_adaptive")] = lambda: ctx.encode_blocks_device(data["sorted int64 keys, delta, split"], BLOCK, dst, offs)

    # warm-up and a check of what is measured: the costs of the numpy mirror on the first two blocks and the last
    for _ in range(2):
        for fn in things.values():
            fn()
    ctx.sync_status()
    for name, src in data.items():
        want = stats.cost_numpy(np.stack([np.bincount(src[b * BLOCK: (b + 1) * BLOCK].cpu().numpy(), minlength=256) for b in (0, 1, nb - 1)]))
        stats.blocks_device(ctx, src, BLOCK, None, d_cost)
        got = d_cost[[0, 1, nb - 1]].cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), (name, got, want)
    assert set(choice) == {"delta"}, choice

    ms = {k: [] for k in things}
    for _ in range(args.repeats):  # one of each per round, in turn
        for key, fn in things.items():
            ms[key].append(once(fn))
    ctx.sync_status()

    rows = []
    med = {k: statistics.median(v) for k, v in ms.items()}
    first = next(iter(data))
    for name in data:
        row = {"part": "stats", "bytes": n, "block": BLOCK, "data": name, "outputs": "cost"}
        for what in ("stats_merged", "crc32"):
            row[what] = summary(ms[(name, what)], n)
        for what in ("stats_merged",):
            row[what + "_over_crc"] = round(med[(name, what)] / med[(name, "crc32")], 3)
            row[what + "_over_uniform"] = round(med[(name, what)] / med[(first, what)], 3)
        rows.append(row)
    a, e = ("sorted int64 keys", "auto_decision"), ("sorted int64 keys", "encode_adaptive")
    rows.append({"part": "auto", "bytes": n, "block": BLOCK, "width": 8, "data": "sorted int64 keys", "choice": choice[-1],
                 "what": "three splits, three statistics passes, one download of three sums; beside one adaptive encode of the split text",
                 "auto_decision": summary(ms[a], n), "encode_adaptive": summary(ms[e], n), "decision_over_encode": round(med[a] / med[e], 4)})
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
