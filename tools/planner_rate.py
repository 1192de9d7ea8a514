#!/usr/bin/env python3
"""The five device-planned calls, this build against the PARENT commit's library, for a change that is meant to leave their
speed alone (DESIGN.md section 25 quotes profiles/r26_planner_rate.jsonl).  Per call part A's batch of its own tool (200 000
ragged entries), the passes of the two builds alternated, 2 warm-up passes, 7 passes, median and min-max: the GPU time of the
call (device events around it) and the planner alone (RCX_T_SCAN) where the call reports it.  Bar: this build's median is no
more than the parent's median plus the parent's own min-max spread in this run.

    python tools/planner_rate.py --baseline-library PATH [--out profiles/r26_planner_rate.jsonl] [--repeats 7]

Each library is served by a process of its own (this tool again with --serve and RCX_LIBRARY set): a process binds one library
through the Python modules, and with this build in the measuring process and the parent in a served one, the same build on
both sides differed by up to 0.011 ms between the two processes.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from base_picks_rate import Parent, Ragged as BaseJoin, alternated, barred, spread, timed  # noqa: E402

CALLS = ("decode", "encode", "typed_join", "base_join", "typed_split")


def workload(name):
    """Part A's batch of the call's own tool, on the library this process binds, its context timing."""
    import encode_picks_rate
    import picks_rate
    import typed_picks_rate
    import typed_split_picks_rate
    from cpprcoder_amd import base_items, base_picks, rcx
    w = {"decode": picks_rate.SmallItems, "encode": lambda: encode_picks_rate.SmallItems(None), "typed_join": lambda: typed_picks_rate.Ragged(rcx.Context(0)),
         "base_join": lambda: BaseJoin(rcx.Context(0), base_items, base_picks), "typed_split": lambda: typed_split_picks_rate.Ragged(rcx.Context(0))}[name]()
    w.ctx.set_timing(True)
    return w


def serve():
    """Requests on stdin, one a line: a call's name prepares its batch, `go` runs one pass and answers `wall_ms gpu_ms`, `scan`
    answers the planner's ms of that pass, `check` synchronises the context, `quit` ends."""
    w = None
    for line in sys.stdin:
        words = line.split()
        if not words or words[0] == "quit":
            break
        if words[0] == "go":
            print(*timed(w.device_planned), flush=True)
        elif words[0] == "scan":
            print(w.ctx.get_timing(reset=True)["scan"]["ms"], flush=True)
        elif words[0] == "check":
            w.ctx.sync_status()
            print("ok", flush=True)
        else:
            w = workload(words[0])
            print("ready", flush=True)


class Served(Parent):
    """A serving process: this tool on the library at `path`."""

    def __init__(self, path):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], env=dict(os.environ, RCX_LIBRARY=path), stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-library")
    ap.add_argument("--serve", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.serve:
        return serve()
    builds = {"this": Served(os.path.join(ROOT, "cpprcoder_amd", "librcx.so")), "parent": Served(os.path.abspath(args.baseline_library))}
    for name in CALLS:
        for b in builds.values():
            b.prepare(name)
        t = alternated({k: b.go for k, b in builds.items()}, args.repeats, after=lambda k: float(builds[k].ask("scan")))
        row = {"call": name, "entries": 200_000, "served_by": "each library by a process of its own"}
        for k, v in t.items():
            builds[k].check()
            row[k] = {"gpu_ms": spread(v["gpu_ms"]), "planner_ms": spread(v["after"])}
        barred(row, row["this"]["gpu_ms"], row["parent"]["gpu_ms"], "this build's GPU median <= the parent's median + the parent's min-max spread of this run")
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    for b in builds.values():
        b.close()


if __name__ == "__main__":
    main()
