"""What the base item tests share (tests/test_base_items_cpu.py, tests/test_gpu_base_items.py): batches of items with a
predictor, a base op or neither around every switch point of the kernels (csrc/rcx_base_items.hpp), where their base spans
lie, their bytes in every data kind.  The expectation is the package's numpy statement (cpprcoder_amd/base_items.py), which
the CPU tests hold to base.py and typed_items.py item by item.  Not a test file."""
import numpy as np

import planes_cases as pc
import typed_items_cases as tc
from cpprcoder_amd import base_items as bi

WIDTHS = (1, 2, 4, 8)
NO_BASE = bi.NO_BASE
OPS = (bi.XOR, bi.SUB, bi.SUBZZ)
OFFSETS = pc.OFFSETS
ROWS = {1: 8, 2: 4, 4: 2, 8: 1}  # RCX_BASE_ROWS(width): rows of 256 units a workgroup of rcx_base_items_k takes at a time
KINDS = ("random", "equal", "plus_minus_one", "most_negative")
LAYOUTS = ("packed", "reverse", "one")  # where the base spans lie: in item order, in reverse order, all at offset 0

# every kind of item: (width, predictor, op) -- 10 with a predictor or nothing (width 1 has no predictor), 12 with an op
ITEM_KINDS = [(w, p, NO_BASE) for w in WIDTHS for p in tc.preds_of(w)] + [(w, 0, op) for w in WIDTHS for op in OPS]


def switch_lengths(w):
    """Item lengths in bytes around every switch point of rcx_base_items_k for width w: typed_items_cases.switch_lengths with the
    workgroup step of the base classes, RCX_BASE_ROWS(w) * 256 * 16 elements, +- one element, and two steps and a unit."""
    step = ROWS[w] * 256 * 16
    elements = [1024 - 1, 1024, 1024 + 1, 4096 - 1, 4096, 4096 + 1, step - 1, step, step + 1, 2 * step + 16 + 5]
    out = [0, 1, w - 1, w, 16 * w - 1, 16 * w, 16 * w + 1, 17 * 16 * w]
    out += [e * w for e in elements]
    out += [e * w + (k % w) for k, e in enumerate(elements, 1) if w > 1]
    return [n for n in out if n >= 0]


def _case(name, items, k, layout=None):
    cols = [np.array([it[j] for it in items], dtype) for j, dtype in ((0, np.uint64), (1, np.uint8), (2, np.uint8), (3, np.uint8))]
    return {"name": name, "lengths": cols[0], "widths": cols[1], "preds": cols[2], "ops": cols[3], "layout": layout or LAYOUTS[k % 3],
            "src_offset": OFFSETS[k % 5], "base_offset": OFFSETS[(k // 5 + k) % 5], "dst_offset": OFFSETS[(k // 25 + 2 * k) % 5]}


def kernel_cases():
    """A list of batches: dict(name, lengths, widths, preds, ops, layout, src_offset, base_offset, dst_offset).  The three offsets
    cycle through (0, 1, 3, 8, 15) independently of one another."""
    out = []
    for w in WIDTHS:  # one class a batch, every switch length
        for op in OPS:
            out.append(_case(f"switch w={w} op={op}", [(n, w, 0, op) for n in switch_lengths(w)], len(out)))
    rs = np.random.RandomState(7)
    kinds = ITEM_KINDS
    out.append(_case("mixed small", [(int(rs.randint(0, 6 * 16 * w + w)), w, p, op) for k in range(700) for (w, p, op) in [kinds[k % len(kinds)]]], len(out)))
    out.append(_case("mixed many", [(int(rs.randint(16 * w, 1024 + w)), w, p, op) for k in range(6000) for (w, p, op) in [kinds[(k * 7) % len(kinds)]]],
                     len(out)))
    run = [(0, 4, 0, bi.SUB)] * 70
    out.append(_case("empty runs", run + [(100, 2, 0, bi.SUBZZ)] + run + [(0, 1, 0, NO_BASE)] * 3 + [(4099, 8, bi.DELTA, NO_BASE), (33, 1, 0, bi.XOR)] + run,
                     len(out)))
    out.append(_case("only empty", run, len(out)))
    out.append(_case("no items", [], len(out)))
    out.append(_case("none with a base", [(int(rs.randint(0, 3000)), w, p, op) for (w, p, op) in kinds[:10] * 3], len(out)))
    out.append(_case("all with a base", [(int(rs.randint(0, 3000)), w, p, op) for (w, p, op) in kinds[10:] * 3], len(out)))
    # large and small side by side: a row that begins in a large item and ends in small ones, and the other way
    out.append(_case("large and small", [(5, 2, 0, bi.SUB), (2 * 4099, 2, 0, bi.SUB), (64, 2, 0, bi.SUB), (7, 2, 0, bi.SUB), (2 * 300, 2, 0, bi.SUB),
                                         (2 * 5000, 2, 0, bi.SUB), (31, 2, 0, bi.SUB)]
                     + [(4 * 16 * 255, 4, 0, bi.SUBZZ), (4 * 16, 4, 0, bi.SUBZZ), (4 * 16 * 3 + 3, 4, 0, bi.SUBZZ)]
                     + [(8 * 16 * 511, 8, 0, bi.XOR), (8 * 16 * 2, 8, 0, bi.XOR)] + [(16 * 2047, 1, 0, bi.SUBZZ), (16, 1, 0, bi.SUBZZ), (40, 1, 0, bi.SUBZZ)], len(out)))
    # KV pages against one reference page: many items, ONE base span
    out.append(_case("many on one span", [(4096 - (k % 3), 2, 0, bi.SUBZZ) for k in range(40)] + [(4096, 1, 0, bi.XOR)] * 8, len(out), "one"))
    out.append(_case("reverse order", [(int(rs.randint(1, 5000)), w, p, op) for (w, p, op) in kinds * 2], len(out), "reverse"))
    k = len(out)
    while len(out) < k + 8 or len(out) % 5:  # (more pairs of offsets)
        out.append(_case(f"offsets {len(out)}", [(int(rs.randint(0, 3000)), w, p, op) for (w, p, op) in kinds], len(out)))
    return out


def offsets_of(case, first=0):
    offs = np.zeros(len(case["lengths"]) + 1, np.uint64)
    np.cumsum(case["lengths"], out=offs[1:])
    return offs + np.uint64(first)


def base_layout(case, first=0):
    """-> (base_offsets uint64[nitems], bytes of the base behind `first`).  An item without an op gets an offset far outside, which
    nobody may look at."""
    lens = case["lengths"].astype(np.int64)
    based = case["ops"] != NO_BASE
    boffs = np.full(len(lens), (1 << 62) + 12345, np.uint64)
    if case["layout"] == "one":
        boffs[based] = first
        return boffs, int(lens[based].max()) if based.any() else 0
    order = np.flatnonzero(based)
    if case["layout"] == "reverse":
        order = order[::-1]
    at = 0
    for i in order:
        boffs[i] = first + at
        at += int(lens[i])
    return boffs, at


def case_data(case, kind, noise):
    """-> (source, base) as uint8 arrays, the batch's bytes and the base's.  random: independent noise.  For the items with an op
    -- equal: the source is the base span; plus_minus_one: element = base element - 1 and + 1 in turn, the borrow and the carry
    through every byte; most_negative: element = base element + 2^(8w - 1), the one difference whose zigzag is all ones.  Tail
    bytes and the items without an op stay noise."""
    total = int(case["lengths"].sum())
    boffs, nbase = base_layout(case)
    x, ref = noise[:total].copy(), noise[total + 7: total + 7 + nbase].copy()
    if kind == "random":
        return x, ref
    at = 0
    for i, (n, w, op) in enumerate(zip(case["lengths"].astype(np.int64), case["widths"], case["ops"])):
        n, w = int(n), int(w)
        m = n // w
        if op != NO_BASE and m:
            dtype = np.dtype(f"<u{w}")
            b = ref[int(boffs[i]): int(boffs[i]) + m * w].view(dtype)
            if kind == "equal":
                e = b
            elif kind == "plus_minus_one":
                e = b + np.where(np.arange(m) & 1, 1, -1).astype(np.int64).astype(dtype)
            else:
                e = b + dtype.type(1 << (8 * w - 1))
            x[at: at + m * w] = e.astype(dtype).view(np.uint8)
        at += n
    return x, ref


def superblock_items(n, width, block, op):
    """A buffer of n bytes cut into items of width * block bytes, its ragged rest as the last -> (lengths, widths, ops)."""
    lengths, widths, _ = tc.superblock_items(n, width, block, 0)
    return lengths, widths, np.full(len(lengths), op, np.uint8)


def write_cases(path, cases):
    """The batches as the text tests/sim/base_items_san.cpp reads: per batch `nitems first base_first base_bytes`, then a line
    `len width pred op base_offset` per item."""
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for k, c in enumerate(cases):
            first, bfirst = (k * 37) % 101, (k * 53) % 97
            boffs, nbase = base_layout(c, bfirst)
            f.write(f"{len(c['lengths'])} {first} {bfirst} {nbase}\n")
            for n, w, p, op, b in zip(c["lengths"], c["widths"], c["preds"], c["ops"], boffs):
                f.write(f"{int(n)} {int(w)} {int(p)} {int(op)} {int(b)}\n")


# ---- a state dict against the one before it -----------------------------------------------------------------------------------
def state_dicts():
    """-> (named, base, predict): the crafted state dict of the documents and the one before it, numpy arrays.  Two bf16 tensors
    randn * 0.02 moved by randn * 1e-4 (as uint16: numpy has no bf16), one fp32 tensor identical to its base, one tensor the base
    lacks, one sorted int64 tensor that wants the predictor and has no base."""
    import base_cases
    rng = np.random.default_rng(18)
    named, base = {}, {}
    for name, count in (("layer0.weight", 1 << 18), ("layer1.weight", 3 << 16)):
        w = (rng.standard_normal(count) * 0.02).astype(np.float32)
        w2 = (w + rng.standard_normal(count) * 1e-4).astype(np.float32)
        named[name], base[name] = base_cases.bf16_bytes(w2).view(np.uint16).reshape(-1, 256), base_cases.bf16_bytes(w).view(np.uint16).reshape(-1, 256)
    frozen = (rng.standard_normal(1 << 16) * 0.02).astype(np.float32)
    named["embed.frozen"], base["embed.frozen"] = frozen.copy(), frozen
    named["head.new"] = (rng.standard_normal(1 << 16) * 0.02).astype(np.float16)
    named["index.sorted"] = np.sort(rng.integers(0, 1 << 40, 1 << 15)).astype(np.int64)
    return named, base, {"index.sorted": "delta"}


def tensor_items(named, base, block, op=2, predict=None):
    """The items pack_tensors_delta makes of a state dict, without a GPU -> dict(x, ref: the items' and the bases' bytes back to
    back; lengths, widths, preds, ops, base_offsets; first: name -> its first item): every tensor cut into items of
    element size * block bytes, with `op` if the base holds it with the same dtype and shape, else with its predictor."""
    parts, refs, lengths, widths, preds, ops, first = [], [], [], [], [], [], {}
    for name, t in named.items():
        w, n = t.dtype.itemsize, t.nbytes
        count = -(-n // (w * block))
        based = name in base and base[name].dtype == t.dtype and base[name].shape == t.shape
        first[name] = len(lengths)
        parts.append(np.ascontiguousarray(t).reshape(-1).view(np.uint8))
        if based:
            refs.append(np.ascontiguousarray(base[name]).reshape(-1).view(np.uint8))
        lengths += [w * block] * (count - 1) + [n - (count - 1) * w * block]
        widths += [w] * count
        ops += [op if based else NO_BASE] * count
        preds += [0 if based or w == 1 else {None: 0, "delta": 1, "zigzag": 2}[(predict or {}).get(name)]] * count
    out = {"x": np.concatenate(parts), "ref": np.concatenate(refs) if refs else np.zeros(0, np.uint8), "lengths": np.array(lengths, np.uint64),
           "widths": np.array(widths, np.uint8), "preds": np.array(preds, np.uint8), "ops": np.array(ops, np.uint8), "first": first}
    boffs = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(np.where(out["ops"] != NO_BASE, out["lengths"], 0), out=boffs[1:])
    out["base_offsets"] = boffs[:-1]
    return out
