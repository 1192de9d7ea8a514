#!/usr/bin/env python3
"""Generate tests/golden/container_parity.json: what the container layer (cpprcoder_amd/container.py) writes, refuses and
calls, recorded at ONE commit so that a later commit that only rearranges that layer can be held to it byte for byte.

Run it at the commit whose behaviour is the pin -- the parent of the change under test, never the change itself -- and name
that commit (--commit; `git rev-parse --short HEAD` if there is a git checkout).  The cases are tests/container_parity_cases.py:
it uses only public names of `container`, so it runs unchanged on every commit that has them.

    python tests/golden/make_golden_containers.py            # the CPU section: no library, no GPU
    python tests/golden/make_golden_containers.py --gpu      # the GPU section, added to the file's CPU section

The CPU section: header bytes and refusals of the four writers, the four parsers on damaged blobs, the calls that return
without a GPU, the rules of "auto" on small tables, the public names.  The GPU section, per case: SHA-256 and length of every
blob and, per public call, the ordered names of the rcx.Context methods and module device calls it made ("traces") and of its
uploads and downloads ("copies").  tests/test_container_parity_cpu.py and
tests/test_gpu_container_parity.py replay them.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import container_parity_cases as cases  # noqa: E402

PATH = os.path.join(HERE, "container_parity.json")


def head_commit() -> str:
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        raise SystemExit("no git checkout here: name the commit this runs at with --commit")


def gpu_section() -> dict:
    import torch
    from cpprcoder_amd import rcx
    assert torch.cuda.is_available(), "the GPU section needs a GPU"
    out = {}
    ctx = rcx.Context(0)
    try:
        for name, run in cases.gpu_cases().items():
            out[name] = cases.run_gpu_case(run, ctx)
            print(name, {k: len(v) for k, v in out[name]["traces"].items()}, flush=True)
    finally:
        ctx.close()
    return out


def dumps(v, depth: int, indent: int = 0) -> str:
    """JSON with one line per entry down to `depth` levels of dicts, compact below: small, and a diff names the case."""
    if depth == 0 or not isinstance(v, dict) or not v:
        return json.dumps(v, sort_keys=True, separators=(",", ":"))
    pad = " " * (indent + 1)
    return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {dumps(v[k], depth - 1, indent + 1)}" for k in sorted(v)) + "\n" + " " * indent + "}"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="record the GPU section (keeps the file's CPU section)")
    ap.add_argument("--commit", help="the commit this runs at")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    commit = args.commit or head_commit()
    doc = json.load(open(PATH)) if os.path.exists(PATH) else {}
    if args.gpu:
        doc["gpu"] = {"commit": commit, "cases": gpu_section()}
    else:
        doc["cpu"] = {"commit": commit, "sections": cases.cpu_section()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(dumps(doc, 4) + "\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
