"""python -m cpprcoder_amd c|d|t ...  -- compress / decompress / test files with the MI355X block coder.

    python -m cpprcoder_amd c [-b BLOCK] [--blksort | --planes W [--predict delta|zigzag|auto]] [--crc] [--stored [FRACTION]]
                              [--base FILE [--base-op xor|sub|subzz|auto]] [--static | --coder adaptive|static|rans|rans8] IN OUT
                                                               IN -> RCXB container (cpprcoder_amd/layout.py);
                                                               --blksort: the reference's block sort (blksort.h) first;
                                                               --planes W: IN is elements of W = 2, 4 or 8 bytes (bf16,
                                                               fp32, int64 ...), taken apart into byte planes first
                                                               (include/rcx_planes.h) -> RCXT container;
                                                               --predict delta|zigzag (with --planes only): the elements
                                                               are integers with small differences (sorted keys, offsets,
                                                               timestamps, samples): each becomes its difference to the
                                                               one in front first, zigzag for differences of both signs
                                                               (include/rcx_predict.h); unsorted data gets worse by it;
                                                               auto: the one that the order-0 cost of the split text says
                                                               pays off by 1/64 or more, else none (include/rcx_stats.h);
                                                               the line printed names the choice;
                                                               --crc: a CRC-32 per block goes into the container;
                                                               --stored [FRACTION]: a block whose stream does not shrink, or
                                                               by less than FRACTION (0 <= FRACTION < 1) of the block, is
                                                               kept as its raw bytes and decoded by copy
                                                               (include/rcx_stored.h): the container never grows past its
                                                               input, and the line printed says "stored K/N" blocks.  In
                                                               front of IN write --stored=FRACTION, or another option behind it;
                                                               --base FILE: IN differs a little from FILE, which has the same
                                                               size and which the reader holds as well (the checkpoint before,
                                                               the base model, the last snapshot): every element becomes its
                                                               residual against FILE's element first (include/rcx_base.h;
                                                               --base-op: xor, sub, or subzz, the default, the zigzagged
                                                               difference, or auto: the cheapest of the three by the
                                                               measured order-0 cost) -> RCXD container, which carries a CRC-32 per
                                                               block of FILE.  With --planes W the elements are W bytes wide,
                                                               without it 1 byte (fp8, bytes); not with --blksort or
                                                               --predict.  Against an unrelated FILE the container grows
    python -m cpprcoder_amd d [--no-verify] [--base FILE] IN OUT
                                                               container (RCXB, RCXT or RCXD, told apart by the magic; an RCXI
                                                               container holds items, not a file) -> original bytes.
                                                               An RCXD container needs --base FILE, the file it was packed
                                                               against: without it, or with a FILE of another size or
                                                               content, the problem is named on stderr, the exit status is 1
                                                               and OUT is not written.
                                                               A container with checksums
                                                               is verified: on a mismatch the bad block is named on
                                                               stderr, the exit status is 1 and OUT is not written
                                                               (--no-verify: write what the decoder produced)
    python -m cpprcoder_amd t [--crc] [--stored [FRACTION]] [--planes W [--predict delta|zigzag|auto]] [--base BASE [--base-op OP]] FILE...
                                                               the reference harness's row per file
                                                               (|file|ratio|encode|decode|, test/main.cpp:346-356):
                                                               pack, unpack, compare, times incl. PCIe copies;
                                                               --base BASE: each FILE against BASE, as with c and d
"""
import argparse
import sys
import time


CODERS = ("adaptive", "static", "rans", "rans8")  # include/rcx.h: RCX_CODER_*
BASE_OPS = ("xor", "sub", "subzz")                # include/rcx_base.h: RCX_BASE_XOR, RCX_BASE_SUB, RCX_BASE_SUBZZ
PREDICTORS = ("delta", "zigzag", "auto")          # include/rcx_predict.h: RCX_PRED_DELTA, RCX_PRED_ZIGZAG; auto: container.pick_predictor


def _fraction(text: str) -> float:
    """--stored's value: a fraction of the block, 0 <= g < 1."""
    g = float(text)
    if not 0 <= g < 1:
        raise argparse.ArgumentTypeError("a fraction of the block, 0 <= FRACTION < 1")
    return g


class _Parser(argparse.ArgumentParser):
    """Rules argparse has no word for: --predict without --planes is an argument error, and so is --base with --blksort or
    --predict, or --base-op without --base."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if getattr(a, "predict", None) and not a.planes:
            self.error("--predict needs --planes W: the predictor works on elements")
        if getattr(a, "base", None) and (getattr(a, "blksort", False) or getattr(a, "predict", None)):
            self.error("--base goes with --planes W or alone (width 1), not with --blksort or --predict")
        if getattr(a, "base_op", None) and not a.base:
            self.error("--base-op needs --base FILE")
        return a


def parser() -> argparse.ArgumentParser:
    ap = _Parser(prog="python -m cpprcoder_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("c")
    c.add_argument("-b", "--block", type=int, default=65536)
    c.add_argument("--static", action="store_true")
    c.add_argument("--coder", choices=CODERS, default=None)
    first = c.add_mutually_exclusive_group()  # what goes in front of the coder: one of the two, or nothing
    first.add_argument("--blksort", action="store_true")
    first.add_argument("--planes", type=int, choices=(2, 4, 8), default=None, metavar="W")
    c.add_argument("--predict", choices=PREDICTORS, default=None)
    c.add_argument("--crc", action="store_true")
    c.add_argument("--stored", nargs="?", type=_fraction, const=True, default=None, metavar="FRACTION")
    c.add_argument("--base", default=None, metavar="FILE")
    c.add_argument("--base-op", choices=list(BASE_OPS) + ["auto"], default=None)
    c.add_argument("src")
    c.add_argument("dst")
    d = sub.add_parser("d")
    d.add_argument("--no-verify", action="store_true")
    d.add_argument("--base", default=None, metavar="FILE")
    d.add_argument("src")
    d.add_argument("dst")
    t = sub.add_parser("t")
    t.add_argument("-b", "--block", type=int, default=65536)
    t.add_argument("--static", action="store_true")
    t.add_argument("--coder", choices=CODERS, default=None)
    first = t.add_mutually_exclusive_group()  # what goes in front of the coder: one of the two, or nothing
    first.add_argument("--blksort", action="store_true")
    first.add_argument("--planes", type=int, choices=(2, 4, 8), default=None, metavar="W")
    t.add_argument("--predict", choices=PREDICTORS, default=None)
    t.add_argument("--crc", action="store_true")
    t.add_argument("--stored", nargs="?", type=_fraction, const=True, default=None, metavar="FRACTION")
    t.add_argument("--base", default=None, metavar="FILE")
    t.add_argument("--base-op", choices=list(BASE_OPS) + ["auto"], default=None)
    t.add_argument("files", nargs="+")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    from . import container, rcx
    coder = CODERS.index(a.coder) if getattr(a, "coder", None) else (1 if getattr(a, "static", False) else 0)
    ctx = rcx.Context(0)

    base = open(a.base, "rb").read() if getattr(a, "base", None) else None

    def pack(data):
        if base is not None:
            return container.pack_delta(data, base, a.planes or 1, a.block, coder, ctx, checksum=a.crc, stored=a.stored, op=a.base_op or "subzz")
        if a.planes:
            return container.pack_typed(data, a.planes, a.block, coder, ctx, checksum=a.crc, predict=a.predict, stored=a.stored)
        return container.pack(data, a.block, coder, ctx, blksort=a.blksort, checksum=a.crc, stored=a.stored)

    def unpack(blob, verify=True):
        if bytes(blob[:4]) == container.DELTA_MAGIC:
            if base is None:
                raise container.ContainerError("an RCXD container holds a residual: give the file it was packed against with --base FILE")
            return container.unpack_delta(blob, base, ctx, verify=verify)
        if bytes(blob[:4]) == container.TYPED_MAGIC:
            return container.unpack_typed(blob, ctx, verify=verify)
        if bytes(blob[:4]) == container.ITEM_MAGIC:
            raise container.ContainerError("an RCXI container holds items, not one file: container.unpack_items()")
        return container.unpack(blob, ctx, verify=verify)

    def chosen(blob):
        """What --stored kept raw and what --predict auto took, for the line printed: the container itself does not say that
        either was asked for."""
        typed = bytes(blob[:4]) == container.TYPED_MAGIC
        out = ""
        if getattr(a, "stored", None) is not None:
            c = container.parse_delta(blob)["inner"] if bytes(blob[:4]) == container.DELTA_MAGIC else container.parse_typed(blob) if typed else container.parse(blob)
            out += f" stored {0 if c['stored'] is None else int(c['stored'].sum())}/{c['nblocks']}"
        if getattr(a, "predict", None) == "auto":
            out += " predict=" + ("none", "delta", "zigzag")[container.parse_typed(blob)["pred"]]
        return out

    try:
        if a.cmd == "c":
            data = open(a.src, "rb").read()
            blob = pack(data)
            open(a.dst, "wb").write(blob)
            print(f"{a.src}: {len(data)} -> {len(blob)} bytes ({len(blob) / max(len(data), 1):.6f})" + chosen(blob))
        elif a.cmd == "d":
            try:
                blob = open(a.src, "rb").read()
                out = unpack(blob, verify=not a.no_verify)
            except container.ChecksumError as e:
                print(f"{a.src}: {e}; nothing written", file=sys.stderr)
                return 1
            except container.ContainerError as e:
                if bytes(blob[:4]) != container.DELTA_MAGIC:
                    raise
                print(f"{a.src}: {e}; nothing written", file=sys.stderr)  # no base, or one of another size or content
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
                blob = pack(data)
                t1 = time.perf_counter()
                back = unpack(blob)
                t2 = time.perf_counter()
                ok = back == data
                bad += not ok
                print(f"|{path}|{len(blob) / max(len(data), 1):.6f}|{(t1 - t0) * 1e6:.0f}|{(t2 - t1) * 1e6:.0f}|" + chosen(blob) + ("" if ok else " MISMATCH"))
            return 1 if bad else 0
    finally:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
