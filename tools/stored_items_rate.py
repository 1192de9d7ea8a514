#!/usr/bin/env python3
"""Rate of the stored-item mix (csrc/rcx_stored_items.hpp) beside the block mix it is modelled on, on a ragged batch, and what
decoding a tensor container costs with and without stored sub-items: one process, warm-up, >= 5 rounds that alternate between
everything measured, median and min-max.  DESIGN.md section 16 quotes profiles/r14_stored_items_rate.jsonl; never bench.py's
`value`.

    python tools/stored_items_rate.py [--out profiles/r14_stored_items_rate.jsonl] [--repeats 5] [--bytes N] [--items N]

Two ways of timing an item call, as in tools/typed_items_rate.py, both with device events:
  call     an event pair around the call on an idle GPU: the host plan, the upload and the kernels
  kernels  the same pair behind enough queued device copies to cover the plan: the first event fires when the copies end, the
           upload and the kernels are already queued behind it -- the upload and the kernels alone

(A) The yardstick.  The GiB of fp32 randn * 0.02 of tools/stored_rate.py, split at width 4, at 64 KiB and at 16 KiB blocks; the
    adaptive coder's block streams; gain 0.  rcx_stored_mix_device (the parent's kernels, unchanged) beside
    rcx_stored_mix_items_device on the same bytes cut into items of one block each, and the same streams: both move the same
    bytes, the item kernels look an entry's item, position and flag up in tables.  The block mix is timed both ways as well
    (it has no plan: the difference is its launch latency).  `kernels_over_block` = the item kernels' median over the block
    mix's median on an idle GPU, `kernels_over_block_kernels` over the block mix timed behind the copies.
(B) A ragged batch: --items typed items of 0 .. 4096 bytes of the fp32 values, widths 1, 2, 4 and 8 mixed, split per item; the
    adaptive coder's streams of the sub-items; the mix as a call and as kernels only, and the wall time of its enqueue.
(C) Tensor decode: container.unpack_tensors(device="cuda") of a GiB of bf16 randn * 0.02 packed with and without
    stored = 256 / 65536 at 16 KiB and 64 KiB blocks, wall time of the whole call (parse, upload of the payload, decode, join).
Every row is time per call in milliseconds.  Nothing here is a pass mark.
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

from cpprcoder_amd import container, planes, rcx, stored, stored_items, typed_items  # noqa: E402

GIB = float(1 << 30)


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


def measure(things, repeats, warm=2):
    ms = {k: [] for k in things}
    for _ in range(warm):
        for fn in things.values():
            fn()
    for _ in range(repeats):  # one of each per round, in turn
        for name, fn in things.items():
            ms[name].append(fn())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_stored_items_rate.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--items", type=int, default=200_000)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    n = args.bytes // (4 * 65536) * (4 * 65536)  # whole superblocks of fp32 at 64 KiB blocks
    ctx = rcx.Context(0)
    rows = []
    busy_a, busy_b = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(2))

    def behind(fn, copies):
        """fn timed behind `copies` queued device copies of the whole buffer (about half a millisecond a GiB each)."""
        def timed():
            for _ in range(copies):
                busy_b.copy_(busy_a)
            return once(fn)
        return timed

    values = (torch.randn(n // 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(12345)) * 0.02).to(torch.float32)
    d_values = values.view(torch.uint8)

    # ---- (A) ------------------------------------------------------------------------------------------------------------
    for block in (65536, 16384):
        src = torch.empty(n, dtype=torch.uint8, device="cuda")
        planes.split_device(ctx, d_values, 4, block, src)
        nb = rcx.block_count(n, block)
        comp = torch.empty(rcx.encode_bound(n, block), dtype=torch.uint8, device="cuda")
        offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
        ctx.encode_blocks_device(src, block, comp, offs)
        ctx.sync_status()
        soffs = np.minimum(np.arange(nb + 1, dtype=np.uint64) * np.uint64(block), np.uint64(n))
        out = {k: (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.zeros(nb + 1, dtype=torch.int64, device="cuda"),
                   torch.zeros(nb, dtype=torch.uint8, device="cuda")) for k in ("block", "items")}
        block_mix = lambda: stored.mix_device(ctx, src, block, comp, comp.numel(), offs, 0, *out["block"])  # noqa: E731
        items_mix = lambda: stored_items.mix_items_device(ctx, src, soffs, comp, comp.numel(), offs, 0, *out["items"])  # noqa: E731
        block_mix()
        items_mix()
        ctx.sync_status()
        total = int(out["block"][1][-1])
        assert torch.equal(out["block"][1], out["items"][1]) and torch.equal(out["block"][2], out["items"][2])  # what is measured writes the same
        assert torch.equal(out["block"][0][:total], out["items"][0][:total])
        cover = 24  # queued copies in front of the kernels-alone timing: above 10 ms, more than the plan of 65 536 items takes
        ms = measure({"block_call": lambda: once(block_mix), "block_kernels": behind(block_mix, cover), "items_call": lambda: once(items_mix),
                      "items_kernels": behind(items_mix, cover)}, args.repeats)
        ctx.sync_status()
        med = {k: statistics.median(v) for k, v in ms.items()}
        rows.append({"part": "A", "bytes": n, "block": block, "items": nb, "coder": "adaptive", "gain": 0, "data": "fp32 randn * 0.02, split at width 4",
                     "coded_bytes": int(offs[-1]), "mixed_bytes": total, "stored": int(out["items"][2].sum()), **{k: stats(v, n) for k, v in ms.items()},
                     "kernels_over_block": round(med["items_kernels"] / med["block_call"], 3),
                     "kernels_over_block_kernels": round(med["items_kernels"] / med["block_kernels"], 3),
                     "call_over_block": round(med["items_call"] / med["block_call"], 3)})
        print(json.dumps(rows[-1]), flush=True)
        del src, comp, offs, out

    # ---- (B) ------------------------------------------------------------------------------------------------------------
    rs = np.random.RandomState(14)
    count = args.items
    lengths = rs.randint(0, 4097, count).astype(np.uint64)
    widths = np.array((1, 2, 4, 8), np.uint8)[rs.randint(0, 4, count)]
    offs_items = rcx.item_offsets(lengths)
    total = int(offs_items[-1])
    assert total <= n
    sub = typed_items.sub_offsets(offs_items, widths)
    nsub = len(sub) - 1
    text = torch.empty(total, dtype=torch.uint8, device="cuda")
    typed_items.split_device(ctx, d_values[:total], offs_items, widths, None, text)
    comp = torch.empty(max(rcx.encode_items_bound(sub, 0), 1), dtype=torch.uint8, device="cuda")
    offs = torch.zeros(nsub + 1, dtype=torch.int64, device="cuda")
    ctx.encode_items_device(text, sub, comp, offs)
    ctx.sync_status()
    mixed, moffs, flags = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.zeros(nsub + 1, dtype=torch.int64, device="cuda"), torch.zeros(nsub, dtype=torch.uint8, device="cuda")
    mix = lambda: stored_items.mix_items_device(ctx, text, sub, comp, comp.numel(), offs, 0, mixed, moffs, flags)  # noqa: E731

    def enqueue_wall():  # the call's host side alone: wall time of the enqueue, the GPU idle before and waited for after
        torch.cuda.synchronize()
        t = time.perf_counter()
        mix()
        ms_ = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        return ms_

    mix()
    ctx.sync_status()
    k = 3000  # the first sub-items against the mirror
    h_offs, h_moffs = offs[: k + 1].cpu().numpy().astype(np.uint64), moffs[: k + 1].cpu().numpy().astype(np.uint64)
    want = stored_items.mix_items_numpy(text[: int(sub[k])].cpu().numpy(), sub[: k + 1], comp[: int(h_offs[-1])].cpu().numpy(), h_offs, 0)
    assert np.array_equal(want[1], h_moffs) and np.array_equal(want[2], flags[:k].cpu().numpy()) and np.array_equal(want[0], mixed[: int(h_moffs[-1])].cpu().numpy())
    cover = 120  # the plan of three quarters of a million sub-items takes tens of milliseconds
    ms = measure({"mix_call": lambda: once(mix), "mix_kernels": behind(mix, cover), "mix_enqueue_wall": enqueue_wall}, args.repeats, warm=1)
    ctx.sync_status()
    rows.append({"part": "B", "items": count, "sub_items": nsub, "bytes": total, "lengths": "0..4096 uniform, RandomState(14)", "widths": "1, 2, 4, 8 mixed",
                 "data": "fp32 randn * 0.02, split per item", "coder": "adaptive", "gain": 0, "coded_bytes": int(offs[-1]), "mixed_bytes": int(moffs[-1]),
                 "stored": int(flags.sum()), **{k_: stats(v, None if k_ == "mix_enqueue_wall" else total) for k_, v in ms.items()}})
    print(json.dumps(rows[-1]), flush=True)
    del text, comp, offs, mixed, moffs, flags, busy_a, busy_b, values, d_values

    # ---- (C) ------------------------------------------------------------------------------------------------------------
    t = (torch.randn(n // 2, device="cuda", generator=torch.Generator("cuda").manual_seed(12345)) * 0.02).to(torch.bfloat16)
    blobs = {}
    for block in (16384, 65536):
        for name, option in (("plain", None), ("stored", 256 / 65536)):
            blobs[(block, name)] = container.pack_tensors({"t": t}, block=block, ctx=ctx, stored=option)

    def unpack(blob):
        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = container.unpack_tensors(blob, device="cuda", ctx=ctx)
            torch.cuda.synchronize()
            ms_ = (time.perf_counter() - t0) * 1e3
            assert back["t"].shape == t.shape
            return ms_
        return timed

    for key, blob in blobs.items():
        assert torch.equal(container.unpack_tensors(blob, device="cuda", ctx=ctx)["t"], t), key
    ms = measure({key: unpack(blob) for key, blob in blobs.items()}, args.repeats, warm=1)
    for block in (16384, 65536):
        c = container.parse_typed_items(blobs[(block, "stored")])
        plain = container.parse_typed_items(blobs[(block, "plain")])
        marks = c.get("stored")
        rows.append({"part": "C", "bytes": n, "block": block, "dtype": "bfloat16", "data": "randn * 0.02", "coder": "adaptive", "gain": 256, "sub_items": int(c["nsub"]),
                     "stored": 0 if marks is None else int(marks.sum()), "payload_plain": len(plain["payload"]), "payload_stored": len(c["payload"]),
                     "unpack_plain_wall": stats(ms[(block, "plain")], n), "unpack_stored_wall": stats(ms[(block, "stored")], n),
                     "stored_over_plain": round(statistics.median(ms[(block, "stored")]) / statistics.median(ms[(block, "plain")]), 3)})
        print(json.dumps(rows[-1]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
