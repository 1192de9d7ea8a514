"""python -m cpprcoder_amd c|d|t ...  -- compress / decompress / test files with the MI355X block coder.

    python -m cpprcoder_amd c [-b BLOCK] [--blksort] [--crc] [--static | --coder adaptive|static|rans|rans8] IN OUT
                                                               IN -> RCXB container (cpprcoder_amd/container.py);
                                                               --blksort: the reference's block sort (blksort.h) first;
                                                               --crc: a CRC-32 per block goes into the container
    python -m cpprcoder_amd d [--no-verify] IN OUT             container -> original bytes.  A container with checksums
                                                               is verified: on a mismatch the bad block is named on
                                                               stderr, the exit status is 1 and OUT is not written
                                                               (--no-verify: write what the decoder produced)
    python -m cpprcoder_amd t [--crc] FILE...                  the reference harness's row per file
                                                               (|file|ratio|encode|decode|, test/main.cpp:346-356):
                                                               pack, unpack, compare, times incl. PCIe copies
"""
import argparse
import sys
import time


CODERS = ("adaptive", "static", "rans", "rans8")  # include/rcx.h: RCX_CODER_*


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cpprcoder_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("c")
    c.add_argument("-b", "--block", type=int, default=65536)
    c.add_argument("--static", action="store_true")
    c.add_argument("--coder", choices=CODERS, default=None)
    c.add_argument("--blksort", action="store_true")
    c.add_argument("--crc", action="store_true")
    c.add_argument("src")
    c.add_argument("dst")
    d = sub.add_parser("d")
    d.add_argument("--no-verify", action="store_true")
    d.add_argument("src")
    d.add_argument("dst")
    t = sub.add_parser("t")
    t.add_argument("-b", "--block", type=int, default=65536)
    t.add_argument("--static", action="store_true")
    t.add_argument("--coder", choices=CODERS, default=None)
    t.add_argument("--blksort", action="store_true")
    t.add_argument("--crc", action="store_true")
    t.add_argument("files", nargs="+")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    from . import container, rcx
    coder = CODERS.index(a.coder) if getattr(a, "coder", None) else (1 if getattr(a, "static", False) else 0)
    ctx = rcx.Context(0)
    try:
        if a.cmd == "c":
            data = open(a.src, "rb").read()
            blob = container.pack(data, a.block, coder, ctx, blksort=a.blksort, checksum=a.crc)
            open(a.dst, "wb").write(blob)
            print(f"{a.src}: {len(data)} -> {len(blob)} bytes ({len(blob) / max(len(data), 1):.6f})")
        elif a.cmd == "d":
            try:
                out = container.unpack(open(a.src, "rb").read(), ctx, verify=not a.no_verify)
            except container.ChecksumError as e:
                print(f"{a.src}: {e}; nothing written", file=sys.stderr)
                return 1
            open(a.dst, "wb").write(out)
            print(f"{a.src}: {len(out)} bytes")
        else:
            print("|file|ratio|encode (microseconds)|decode (microseconds)|")
            print("|:---|:---|:---|:---|")
            bad = 0
            for path in a.files:
                data = open(path, "rb").read()
                t0 = time.perf_counter()
                blob = container.pack(data, a.block, coder, ctx, blksort=a.blksort, checksum=a.crc)
                t1 = time.perf_counter()
                back = container.unpack(blob, ctx)
                t2 = time.perf_counter()
                ok = back == data
                bad += not ok
                print(f"|{path}|{len(blob) / max(len(data), 1):.6f}|{(t1 - t0) * 1e6:.0f}|{(t2 - t1) * 1e6:.0f}|" + ("" if ok else " MISMATCH"))
            return 1 if bad else 0
    finally:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
