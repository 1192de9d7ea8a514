"""The candidate costs on the GPU (include/rcx_typed_stats.h; csrc/rcx_typed_stats.hpp) against the numpy mirror
(cpprcoder_amd/typed_stats.py: costs_numpy), exactly, and the containers that decide with them against the named choices, byte
for byte.

rcx_typed_stats_k<W> gives a workgroup to an item: a lane's unit is 16 elements, a wave's pass 64 units, a workgroup's 256, one
row in flight; what is not a unit goes an element and a byte a lane.  The batches (tests/typed_stats_cases.py) sit on both
sides of every border of that for every width, with every mask a width may ask for, the base spans in item order, in reverse
order and all in one place, source and base at offsets from (0, 1, 3, 8, 15), every buffer and the table between guard bytes,
in six kinds of data; then mixed widths and masks over a few thousand items and one of 4 MiB, and 65 535 to 65 537 tiny items,
where the grid loops."""
import numpy as np
import pytest

import base_items_cases as bc
import typed_stats_cases as tsc
from cpprcoder_amd import container, rcx, typed_stats as ts
from gpu_support import Guarded, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def noise():
    return np.random.RandomState(20262).randint(0, 256, (24 << 20) + 64, dtype=np.uint8)


def run(ctx, x, ref, offs, boffs, widths, masks, src_offset=0, base_offset=0, cost_offset=0, status=rcx.OK):
    """One device call with source, base and table guarded -> the table uint64 [nitems, 6]; source and base unchanged, nothing
    but the table's 48 bytes an item written.  With another `status` the call must return it and write nothing."""
    nitems = len(widths)
    src, their = Guarded(len(x), src_offset, x, salt=1), Guarded(len(ref), base_offset, ref, salt=5)
    cost = Guarded(48 * nitems, cost_offset, salt=2)
    assert cost_offset % 8 == 0
    table = cost.view.view(torch.int64)
    if status != rcx.OK:
        with pytest.raises(rcx.RcxError) as e:
            ts.items_device(ctx, src.view, their.view, offs, boffs, widths, masks, table)
        assert e.value.status == status
    else:
        ts.items_device(ctx, src.view, their.view, offs, boffs, widths, masks, table)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK
    src.check(0, "the source")
    their.check(0, "the base")
    cost.check(48 * nitems if status == rcx.OK else 0, "the table")
    return cost.view.cpu().numpy().view(np.uint64).reshape(nitems, 6)


def compare(got, want, masks, label):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (label, bad[:6].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    asked = (np.asarray(masks)[:, None] >> np.arange(6)) & 1
    assert not got[asked == 0].any(), label  # what was not asked for is 0


# ---- the kernel against numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", tsc.WIDTHS)
def test_every_switch_length_and_mask_against_numpy(ctx, noise, width):
    for k, mask in enumerate(tsc.masks_of(width)):
        lengths, widths, masks, layout = tsc.width_batch(width, mask, tsc.LAYOUTS[k % 3])
        offs, (boffs, _) = tsc.offsets_of(lengths), tsc.layout_of(lengths, masks, layout)
        x, ref = tsc.data_of(lengths, widths, masks, layout, "random", noise[k:])
        so, bo = tsc.OFFSETS[k % 5], tsc.OFFSETS[(k + 2) % 5]
        got = run(ctx, x, ref, offs, boffs, widths, masks, so, bo, 8 * (k & 1))
        compare(got, ts.costs_numpy(x, ref, offs, boffs, widths, masks), masks, (width, mask, layout, so, bo))


@pytest.mark.parametrize("kind", tsc.KINDS)
def test_kinds_of_data_against_numpy(ctx, noise, kind):
    """Equal to the base, plus and minus one, the most negative difference, a constant item, two alternating values: the skewed
    tables.  Lengths around the unit and the passes, without the two long ones."""
    for k, width in enumerate(tsc.WIDTHS):
        lengths, widths, masks, layout = tsc.width_batch(width, ts.ALL_OPS if width == 1 else ts.ALL, tsc.LAYOUTS[k % 3])
        keep = lengths < 65536
        lengths, widths, masks = lengths[keep], widths[keep], masks[keep]
        offs, (boffs, _) = tsc.offsets_of(lengths), tsc.layout_of(lengths, masks, layout)
        x, ref = tsc.data_of(lengths, widths, masks, layout, kind, noise[100 + k:])
        got = run(ctx, x, ref, offs, boffs, widths, masks, tsc.OFFSETS[(k + 1) % 5], tsc.OFFSETS[(k + 3) % 5])
        compare(got, ts.costs_numpy(x, ref, offs, boffs, widths, masks), masks, (kind, width, layout))


def test_mixed_widths_and_masks_and_one_long_item(ctx, noise):
    lengths, widths, masks, layout = tsc.mixed_batch(2000, 7, longest=4 << 20)
    widths[1000], masks[1000] = 4, ts.ALL
    offs, (boffs, _) = tsc.offsets_of(lengths), tsc.layout_of(lengths, masks, layout)
    x, ref = tsc.data_of(lengths, widths, masks, layout, "plus_minus_one", noise)
    got = run(ctx, x, ref, offs, boffs, widths, masks, 3, 1)
    compare(got, ts.costs_numpy(x, ref, offs, boffs, widths, masks), masks, "mixed")
    # the host-buffer call gives the same table
    assert np.array_equal(ts.items(ctx, x, ref, offs, boffs, widths, masks), got)


@pytest.fixture(scope="module")
def many(noise):
    """65 537 items of 0 to 5 bytes, widths and masks mixed: a pattern of 251 items over and over, all repetitions against the
    pattern's base spans, so the mirror runs once over the pattern and the expectation is its table repeated; fewer items are a
    prefix of it."""
    rs = np.random.RandomState(67)
    period, count = 251, 65537
    lengths = rs.randint(0, 6, period).astype(np.uint64)
    widths = np.array(tsc.WIDTHS, np.uint8)[rs.randint(0, 4, period)]
    masks = np.array([tsc.masks_of(int(w))[k % len(tsc.masks_of(int(w)))] for k, w in enumerate(widths)], np.uint8)
    offs, (boffs, nbase) = tsc.offsets_of(lengths), tsc.layout_of(lengths, masks, "reverse")
    x, ref = noise[: int(offs[-1])], noise[(4 << 20): (4 << 20) + nbase]
    want = ts.costs_numpy(x, ref, offs, boffs, widths, masks)
    reps = -(-count // period)
    tile = lambda a: np.tile(a, reps if a.ndim == 1 else (reps, 1))[:count]  # noqa: E731
    return tsc.offsets_of(tile(lengths)), tile(boffs), tile(widths), tile(masks), np.tile(x, reps), ref, tile(want)


@pytest.mark.parametrize("nitems", (65535, 65536, 65537))
def test_item_counts_around_two_to_the_sixteen(ctx, many, nitems):
    offs, boffs, widths, masks, x, ref, want = many
    got = run(ctx, x[: int(offs[nitems])], ref, offs[: nitems + 1], boffs[:nitems], widths[:nitems], masks[:nitems], 1, 15, 8)
    compare(got, want[:nitems], masks[:nitems], nitems)


def test_items_inside_a_larger_buffer_and_nothing_to_do(ctx, noise):
    x, ref = noise[5: 20_005], noise[30_000: 36_100]
    offs, boffs = np.array([777, 777 + 4 * 1000 + 3, 9000, 9000, 15_001], np.uint64), np.array([1, 0, 0, 0], np.uint64)
    widths, masks = np.array([4, 2, 8, 1], np.uint8), np.array([ts.ALL, ts.ALL_PREDS, ts.ALL, ts.ALL_OPS], np.uint8)
    got = run(ctx, x, ref, offs, boffs, widths, masks, 3, 1)
    compare(got, ts.costs_numpy(x, ref, offs, boffs, widths, masks), masks, "inside")
    # all masks 0: the table is zeroed; no item: nothing is written; no base at all where no op is asked for
    assert not run(ctx, x, ref, offs, boffs, widths, np.zeros(4, np.uint8)).any()
    assert run(ctx, x, ref, offs[:1], boffs[:0], widths[:0], masks[:0]).shape == (0, 6)
    cost = torch.full((12,), -1, dtype=torch.int64, device="cuda")
    ts.items_device(ctx, torch.from_numpy(x.copy()).cuda(), None, offs[:3], None, widths[:2], np.array([1, ts.ALL_PREDS], np.uint8), cost)
    assert np.array_equal(cost.cpu().numpy().view(np.uint64).reshape(2, 6), ts.costs_numpy(x, None, offs[:3], None, widths[:2], [1, ts.ALL_PREDS]))


def test_every_refusal_writes_nothing(ctx, noise):
    x, ref = noise[:4096], noise[5000:9096]
    offs, boffs, widths, masks = np.array([0, 1000, 4096], np.uint64), np.array([0, 1000], np.uint64), np.array([2, 4], np.uint8), np.array([ts.ALL, ts.ALL], np.uint8)
    bad = rcx.E_ARG
    run(ctx, x, ref, np.array([0, 1000, 999], np.uint64), boffs, widths, masks, status=bad)
    run(ctx, x, ref, offs, boffs, np.array([2, 3], np.uint8), masks, status=bad)
    run(ctx, x, ref, offs, boffs, widths, np.array([0x40, 1], np.uint8), status=bad)
    run(ctx, x, ref, offs, boffs, np.array([1, 4], np.uint8), np.array([2, 1], np.uint8), status=bad)
    run(ctx, x, ref, offs, None, widths, masks, status=bad)
    run(ctx, x, ref, offs, np.array([(1 << 64) - 999, 0], np.uint64), widths, np.array([8, 0], np.uint8), status=bad)
    src, their = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(ref.copy()).cuda()
    cost = torch.zeros(13, dtype=torch.int64, device="cuda")
    lib = ts.lib()

    def call(d_src, d_ref, d_cost, m=masks):
        return lib.rcx_typed_stats_items_device(ctx._h, d_src, d_ref, offs.ctypes.data, boffs.ctypes.data, widths.ctypes.data, m.ctypes.data, 2, d_cost, None)

    assert call(src.data_ptr(), their.data_ptr(), cost.data_ptr()) == rcx.OK
    assert call(src.data_ptr(), their.data_ptr(), None) == bad and call(src.data_ptr(), their.data_ptr(), cost.data_ptr() + 4) == bad  # null, misaligned
    assert call(None, their.data_ptr(), cost.data_ptr()) == bad and call(src.data_ptr(), None, cost.data_ptr()) == bad
    assert call(src.data_ptr(), None, cost.data_ptr(), np.array([7, 7], np.uint8)) == rcx.OK                                         # no op bit: no base needed
    assert call(src.data_ptr(), their.data_ptr(), src.data_ptr() + 4000) == bad and call(src.data_ptr(), their.data_ptr(), their.data_ptr() + 8) == bad  # overlaps
    # the host variant: a span past base_bytes
    with pytest.raises(rcx.RcxError):
        ts.items(ctx, x, ref[:4095], offs, boffs, widths, masks)
    assert ts.items(ctx, x, ref[:4095], offs, boffs, widths, np.array([ts.ALL, 7], np.uint8)).shape == (2, 6)
    assert ctx.sync_status(raise_on_error=False)[0] == rcx.OK


def test_the_tables_are_counted_as_scratch(noise):
    """rcx_ctx_scratch_bytes counts the call's tables: a fresh context holds at least their 25 bytes an item behind a call."""
    from gpu_support import context
    nitems = 4000
    lengths, widths, masks = np.full(nitems, 3, np.uint64), np.full(nitems, 2, np.uint8), np.full(nitems, ts.ALL, np.uint8)
    offs = tsc.offsets_of(lengths)
    own = context()
    try:
        before = own.scratch_bytes()
        cost = torch.zeros(6 * nitems, dtype=torch.int64, device="cuda")
        src = torch.from_numpy(noise[: 3 * nitems].copy()).cuda()
        ts.items_device(own, src, src, offs, offs[:-1], widths, masks, cost)
        assert own.sync_status(raise_on_error=False)[0] == rcx.OK
        assert own.scratch_bytes() >= max(before, 25 * nitems) and before < 25 * nitems
    finally:
        own.close()
    got = cost.cpu().numpy().view(np.uint64).reshape(nitems, 6)
    assert np.array_equal(got[:50], ts.costs_numpy(noise[:150], noise[:150], offs[:51], offs[:50], widths[:50], masks[:50]))
    assert set(np.unique(got).tolist()) <= {0, 131072}  # one element and a tail byte: the last plane's two bytes are equal or not


# ---- the decision and the containers ---------------------------------------------------------------------------------------------
def test_the_decision_on_the_gpu_is_the_cpu_decision(ctx):
    for name, data, base, width, pick, tie in tsc.table_rows():
        x, offs, widths, masks = tsc.row_tables(data, width)
        ref = np.ascontiguousarray(base).reshape(-1).view(np.uint8)
        items = [x[int(offs[i]): int(offs[i + 1])] for i in range(len(widths))]
        bases = [ref[int(offs[i]): int(offs[i + 1])] for i in range(len(widths))]
        predict = "auto" if width > 1 else None
        costs = ts.costs_numpy(x, ref, offs, offs[:-1], widths, masks)
        want = container.choose_delta_items_from_costs(costs, [True] * len(widths), widths, "auto", predict)
        assert container.choose_delta_items(items, bases, int(width), "auto", predict, ctx) == want, name
        assert set(want[0]) | set(want[1]) == {pick, None}, name
    named, before, _ = bc.state_dicts()
    m = container.tensor_delta_masks(named, before, 65536, "auto", "auto")
    t = bc.tensor_items(named, before, 65536)
    costs = ts.costs_numpy(t["x"], t["ref"], tsc.offsets_of(t["lengths"]), t["base_offsets"], t["widths"], m["masks"])
    want = container.choose_tensors_delta_from_costs(costs, named, before, 65536, "auto", "auto")
    assert container.choose_tensors_delta(named, before, 65536, "auto", "auto", ctx) == want
    assert want[0]["layer0.weight"] == "subzz" and want[0]["head.new"] is None and want[1]["index.sorted"] == "delta"


def cpu_choice(items, bases, ops, predict):
    """The decision from the mirror's table, the bases of all items that have one back to back."""
    has = [b is not None for b in bases]
    widths = np.array([x.dtype.itemsize for x in items], np.uint8)
    masks = container.delta_item_masks(has, widths, ops, predict)
    lengths = np.array([x.nbytes for x in items], np.uint64)
    x = np.concatenate([v.view(np.uint8) for v in items])
    ref = np.concatenate([b.view(np.uint8) for b in bases if b is not None])
    boffs = tsc.offsets_of(np.where(has, lengths, 0))[:-1]
    return container.choose_delta_items_from_costs(ts.costs_numpy(x, ref, tsc.offsets_of(lengths), boffs, widths, masks), has, widths, ops, predict)


def test_containers_byte_for_byte_against_the_named_choices(ctx):
    rows = {name: (data, base, width) for name, data, base, width, _, _ in tsc.table_rows()}
    # items: a few rows' first 70 000 bytes each as one item, one without a base, one empty
    picks = ("bf16 moved", "bf16 unrelated", "fp32 identical", "sorted int64", "uint8 flipped", "uint64 counters")
    items = [np.ascontiguousarray(rows[n][0]).reshape(-1)[: 70_000 // rows[n][2]] for n in picks]
    bases = [np.ascontiguousarray(rows[n][1]).reshape(-1)[: 70_000 // rows[n][2]] for n in picks]
    items += [items[3].copy(), items[0][:0]]
    bases += [None, bases[0][:0]]
    ops, predict = ["auto"] * 6 + [None, "auto"], ["auto", None, "auto", "auto", None, None, "auto", "auto"]
    chosen = container.choose_delta_items(items, bases, None, ops, predict, ctx)
    assert chosen == cpu_choice(items, bases, ops, predict)
    assert chosen == (["subzz", None, "subzz", None, "xor", "subzz", None, None], [None, None, None, "delta", None, None, "delta", None])
    blob = container.pack_delta_items(items, bases, None, ops, predict, ctx=ctx, checksum=True)
    assert blob == container.pack_delta_items(items, bases, None, chosen[0], chosen[1], ctx=ctx, checksum=True)
    needed = [b if o else None for b, o in zip(bases, chosen[0])]  # the items decided "no base" unpack without theirs
    assert container.unpack_delta_items(blob, needed, ctx=ctx) == [x.tobytes() for x in items]
    scalar = cpu_choice(items, bases, "auto", None)
    assert scalar == (["subzz", None, "subzz", "subzz", "xor", "subzz", None, None], [None] * 8)  # without the predictors the sorted keys lean on their base
    assert container.choose_delta_items(items, bases, None, "auto", None, ctx) == scalar
    each = ["auto" if b is not None else None for b in bases]
    assert container.pack_delta_items(items, bases, None, each, ctx=ctx) == container.pack_delta_items(items, bases, None, scalar[0], ctx=ctx)
    # tensors: the crafted state dict, and a tensor against an unrelated base, which then is not needed to unpack
    named, before, _ = bc.state_dicts()
    named = dict(named, stranger=named["layer0.weight"])
    before = dict(before, stranger=np.random.default_rng(3).integers(0, 1 << 16, named["stranger"].shape).astype(np.uint16))
    op, pred = container.choose_tensors_delta(named, before, 65536, "auto", "auto", ctx)
    assert op["stranger"] is None and op["layer0.weight"] == "subzz" and op["embed.frozen"] == "subzz" and pred["index.sorted"] == "delta"
    blob = container.pack_tensors_delta(named, before, op="auto", predict="auto", ctx=ctx)
    assert blob == container.pack_tensors_delta(named, before, op=op, predict=pred, ctx=ctx)
    back = container.unpack_tensors_delta(blob, {k: v for k, v in before.items() if k != "stranger"}, ctx=ctx)
    assert all(np.array_equal(back[k].numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(v).view(np.uint8).reshape(-1)) for k, v in named.items())
    # one buffer: the cheapest of the three ops
    for name, want in (("bf16 moved", "subzz"), ("uint8 flipped", "xor"), ("fp32 identical", "subzz")):
        data, base, width = rows[name]
        x, ref = np.ascontiguousarray(data).reshape(-1)[: 300_001 // width], np.ascontiguousarray(base).reshape(-1)[: 300_001 // width]
        blob = container.pack_delta(x, ref, block=4096, op="auto", ctx=ctx)
        assert blob == container.pack_delta(x, ref, block=4096, op=want, ctx=ctx), name
        assert container.unpack_delta(blob, ref, ctx=ctx) == x.tobytes()
