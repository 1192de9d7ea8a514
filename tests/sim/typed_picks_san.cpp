// typed_picks_san.cpp -- the planner's rules of cpprcoder_amd/csrc/rcx_typed_picks.hpp (rcx_tpick_validate, rcx_tpick_key,
// rcx_tpick_units, rcx_tpick_bin, and the class planner's rcx_class_head, rcx_class_row: plain functions, the same text the kernels compile) in a
// program of its own, to be built with -fsanitize=address,undefined (tests/test_typed_picks_cpu.py does).  It reads batches of
// entries and what typed_picks.plan_numpy says of them from a file, plans each batch in the planner's steps -- keys and tile
// sums, the sums over the tiles and the head, the places, the rows -- and checks
//   the model     status, position and every entry's route and bin are plan_numpy's
//   the plan      ufirst ascends and is the exact prefix sum of the placed entries' whole units, ufirst[nent] closes it; every
//                 unit of every class, searched between its row's bounds as the kernels search, lies in its own entry; every
//                 row's bound is the entry of the row's first unit and the closing one the class's last entry; the head is what
//                 rcx_typed_plan computes for the same entries; the scan list is in work order
// The tables lie in heap blocks of exactly their size, so a step outside is an error of the sanitizer as well.
// Test tooling, not part of librcx.so.
#include "picks_san.hpp"

namespace
{

// (the model's columns: model0 = the entry's route, model1 = its bin)
bool run(const TypedBatch& b, int which)
{
    const u64 max_pick = b.len.size(), count = b.count < max_pick ? b.count : max_pick, tiles = rcx_tpick_tiles(count);
    u32 flags = 0;
    u64 first_bad = ~0ull;
    auto flag = [&](u32 what, u64 k) {
        flags |= what;
        if (k < first_bad) first_bad = k;
    };
    if (b.count > max_pick) flag(RCX_TPICK_CAPACITY, max_pick);
    // classify: keys, tile sums, bins
    std::vector<u32> keys(max_pick, RCX_TPICK_NONE), bins(RCX_TPICK_BINS, 0);
    std::vector<u64> tile_sum(tiles * 5, 0);
    for (u64 k = 0; k < count; ++k) {
        const u64 len = b.len[k];
        if (len == 0) continue;
        const u32 w = b.widths[k], pr = b.preds[k];
        const u32 bad = rcx_tpick_validate(b.src_at[k], b.dst_at[k], len, w, pr, b.src_cap, b.dst_cap);
        if (bad) {
            flag(bad, k);
            continue;
        }
        keys[k] = rcx_tpick_key((u32)len, w, pr);
        const u64 tile = k / RCX_TPICK_THREADS;
        if (keys[k] < 4u) tile_sum.at(tile * 5 + keys[k]) += sim_value(len, w);
        else bins.at(keys[k] - 4u) += 1;
        tile_sum.at(tile * 5 + 4) += len;
    }
    // top: sums over the tiles, the head, the cursors
    std::vector<u64> tile_units;
    std::vector<u32> tile_ents;
    u64 totals[8];
    const u64 bytes = sim_top<4>(tile_sum, tile_ents, tile_units, totals);
    const bool over = bytes > b.max_bytes;
    if (over) {
        flag(RCX_TPICK_CAPACITY, count);
        for (u64& x : totals) x = 0;
    }
    u64 of_class[2 * RCX_TYPED_CLASSES] = {}; // key c = class 3 c
    for (u32 c = 0; c < 4; ++c) of_class[3 * c] = totals[c], of_class[RCX_TYPED_CLASSES + 3 * c] = totals[4 + c];
    RcxTypedClasses cl;
    memset(&cl, 0, sizeof(cl));
    rcx_class_head(of_class, of_class + RCX_TYPED_CLASSES, [](u32 w) { return RCX_PLANES_U4 / w; }, cl);
    const u32 nent = cl.ent_first[RCX_TYPED_CLASSES];
    std::vector<u32> cursor(RCX_TPICK_BINS, 0);
    u32 nscan = 0;
    for (u32 i = 0; i < RCX_TPICK_BINS; ++i) {
        cursor[i] = nscan;
        nscan += bins[i];
    }
    if (over) nscan = 0;
    // the model
    const int status = (flags & RCX_TPICK_CORRUPT) ? 2 : (flags & RCX_TPICK_CAPACITY) ? 1 : 0; // as the file has it: corrupt, capacity, ok
    CHECK(status == b.status, "status %d, the model says %d", status, b.status);
    CHECK((flags ? (long long)first_bad : -1) == b.position, "position %lld, the model says %lld", flags ? (long long)first_bad : -1, b.position);
    for (u64 k = 0; k < max_pick; ++k) {
        const int route = over || keys[k] == RCX_TPICK_NONE ? 0 : keys[k] < 4u ? 1 : 2;
        CHECK(route == b.model0[k], "entry %llu: route %d, the model says %lld", (unsigned long long)k, route, b.model0[k]);
        const long long bin = keys[k] != RCX_TPICK_NONE && keys[k] >= 4u ? (long long)keys[k] - 4 : -1;
        CHECK(bin == b.model1[k], "entry %llu: bin %lld, the model says %lld", (unsigned long long)k, bin, b.model1[k]);
    }
    if (over) {
        CHECK(nent == 0 && cl.step_end[RCX_TYPED_CLASSES - 1] == 0 && cl.rest_end[RCX_TYPED_CLASSES - 1] == 0, "an overflowing call has work");
        return true;
    }
    // apply: the places
    std::vector<u64> ufirst(nent + 1, ~0ull), len_of(nent, 0);
    std::vector<u32> width_of(nent, 0), scan_len(nscan, 0);
    std::vector<u8> placed(nent, 0);
    for (u64 t = 0; t < tiles; ++t) {
        u64 before[4] = {};
        for (u64 k = t * RCX_TPICK_THREADS; k < count && k < (t + 1) * RCX_TPICK_THREADS; ++k) {
            const u32 key = keys[k];
            if (key == RCX_TPICK_NONE) continue;
            if (key < 4u) {
                const u32 c = 3u * key;
                const u64 place = (u64)cl.ent_first[c] + tile_ents[t * 4 + key] + (before[key] >> RCX_TPICK_COUNT_SHIFT);
                CHECK(place < nent && !placed[place], "entry %llu: place %llu", (unsigned long long)k, (unsigned long long)place);
                placed[place] = 1;
                ufirst[place] = cl.ubase[c] + tile_units[t * 4 + key] + (before[key] & SIM_LOW);
                len_of[place] = b.len[k];
                width_of[place] = b.widths[k];
                before[key] += sim_value(b.len[k], b.widths[k]);
            } else {
                const u32 s = cursor.at(key - 4u)++;
                CHECK(s < nscan, "entry %llu: scan place %u of %u", (unsigned long long)k, s, nscan);
                scan_len[s] = (u32)b.len[k];
            }
        }
    }
    ufirst[nent] = cl.ubase[RCX_TYPED_CLASSES];
    // the plan's invariants
    for (u32 s = 0; s + 1 < nscan; ++s) CHECK(rcx_tpick_bin(scan_len[s]) <= rcx_tpick_bin(scan_len[s + 1]), "the scan list is out of order at %u", s);
    for (u32 s = 0; s < nscan; ++s) CHECK(scan_len[s] > 0, "scan place %u is empty", s);
    for (u32 k = 0; k < nent; ++k) {
        CHECK(placed[k], "place %u is empty", k);
        const u32 c = rcx_typed_class(width_of[k], 0);
        CHECK(k >= cl.ent_first[c] && k < cl.ent_first[c + 1], "place %u is not in its class", k);
        CHECK(ufirst[k + 1] >= ufirst[k] && ufirst[k + 1] - ufirst[k] == rcx_tpick_units((u32)len_of[k], width_of[k]), "ufirst is not the prefix sum at %u", k);
    }
    // the head against the host's plan of the same entries in the placed order
    {
        std::vector<u64> offs(nent + 1, 0), mem;
        std::vector<u8> w(nent);
        for (u32 k = 0; k < nent; ++k) offs[k + 1] = offs[k] + len_of[k], w[k] = (u8)width_of[k];
        RcxTypedPlan p;
        CHECK(rcx_typed_plan(offs.data(), w.data(), nullptr, nent, true, mem, p), "the host plan refuses the entries");
        const RcxTypedTables t = rcx_typed_tables(reinterpret_cast<const u8*>(mem.data()), p);
        CHECK(memcmp(t.classes, &cl, sizeof(cl)) == 0, "the head is not the host plan's");
        CHECK(p.nent == nent && memcmp(t.ufirst, ufirst.data(), (nent + 1) * sizeof(u64)) == 0, "ufirst is not the host plan's");
        // the rows: every one as the host plan has it
        const std::vector<u32> rowtab = sim_rows(cl, ufirst);
        const u32 rows = (u32)rowtab.size();
        CHECK(rows == p.nrows && rows <= rcx_class_rows_most(b.max_bytes, 4u), "%u rows, bound %llu", rows, (unsigned long long)rcx_class_rows_most(b.max_bytes, 4u));
        for (u32 r = 0; r < rows; ++r) CHECK(rowtab[r] == t.rowtab[r], "row %u: entry %u, the host plan has %u", r, rowtab[r], t.rowtab[r]);
        if (!units_found(cl, ufirst, rowtab, which, "typed")) return false;
    }
    return true;
}

} // namespace

int main(int argc, char** argv) { return sim_typed_main<false>(argc, argv, "typed_picks_san", run); }
