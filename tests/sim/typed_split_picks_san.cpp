// typed_split_picks_san.cpp -- the planner's rules of cpprcoder_amd/csrc/rcx_typed_split_picks.hpp (rcx_tpick_validate,
// rcx_typed_class, rcx_tpick_units, rcx_tpick_tiles, and the class planner's rcx_class_head, rcx_class_row: plain functions, the same text the kernels
// compile) in a program of its own, to be built with -fsanitize=address,undefined (tests/test_typed_split_picks_cpu.py does).
// It reads batches of entries and what typed_split_picks.plan_numpy says of them from a file, plans each batch in the planner's
// steps -- keys and tile sums, the sums over the tiles and the head, the places and kept, the rows -- and checks
//   the model     status, position and every entry's class, place and kept are plan_numpy's
//   the plan      ufirst ascends and is the exact prefix sum of the placed entries' whole units, ufirst[nent] closes it; every
//                 unit of every class, searched between its row's bounds as the kernels search, lies in its own entry; every
//                 row's bound is the entry of the row's first unit and the closing one the class's last entry; head, ufirst and
//                 rows are what rcx_typed_plan(..., scan = false) computes for the same entries in the placed order
// The tables lie in heap blocks of exactly their size, so a step outside is an error of the sanitizer as well.
// Test tooling, not part of librcx.so.
#include "picks_san.hpp"

namespace
{

// (the model's columns: model0 = the entry's class, model1 = its place, model2 = its kept)
bool run(const TypedBatch& b, int which)
{
    constexpr u32 NC = RCX_SPICK_KEYS, NS = NC + 1u;
    constexpr u64 LOW = SIM_LOW;
    const u64 max_pick = b.len.size(), count = b.count < max_pick ? b.count : max_pick, tiles = rcx_tpick_tiles(count);
    u32 flags = 0;
    u64 first_bad = ~0ull;
    auto flag = [&](u32 what, u64 k) {
        flags |= what;
        if (k < first_bad) first_bad = k;
    };
    if (b.count > max_pick) flag(RCX_TPICK_CAPACITY, max_pick);
    // classify: keys, tile sums
    std::vector<u32> keys(max_pick, RCX_TPICK_NONE);
    std::vector<u64> tile_sum(tiles * NS, 0);
    for (u64 k = 0; k < count; ++k) {
        const u64 len = b.len[k];
        if (len == 0) continue;
        const u32 w = b.widths[k], pr = b.preds[k];
        const u32 bad = rcx_tpick_validate(b.src_at[k], b.dst_at[k], len, w, pr, b.src_cap, b.dst_cap);
        if (bad) {
            flag(bad, k);
            continue;
        }
        keys[k] = rcx_typed_class(w, pr);
        CHECK(keys[k] < NC, "entry %llu: class %u", (unsigned long long)k, keys[k]);
        const u64 tile = k / RCX_TPICK_THREADS;
        tile_sum.at(tile * NS + keys[k]) += sim_value(len, w);
        tile_sum.at(tile * NS + NC) += len;
    }
    // top: sums over the tiles, the head
    std::vector<u64> tile_units;
    std::vector<u32> tile_ents;
    u64 totals[2 * NC];
    const u64 bytes = sim_top<NC>(tile_sum, tile_ents, tile_units, totals);
    const bool over = bytes > b.max_bytes;
    if (over) {
        flag(RCX_TPICK_CAPACITY, count);
        for (u64& x : totals) x = 0;
    }
    RcxTypedClasses cl;
    memset(&cl, 0, sizeof(cl));
    rcx_class_head(totals, totals + NC, [](u32 w) { return RCX_PLANES_U4 / w; }, cl);
    const u32 nent = cl.ent_first[RCX_TYPED_CLASSES];
    // the model's status and classes
    const int status = (flags & RCX_TPICK_CORRUPT) ? 2 : (flags & RCX_TPICK_CAPACITY) ? 1 : 0; // as the file has it: corrupt, capacity, ok
    CHECK(status == b.status, "status %d, the model says %d", status, b.status);
    CHECK((flags ? (long long)first_bad : -1) == b.position, "position %lld, the model says %lld", flags ? (long long)first_bad : -1, b.position);
    for (u64 k = 0; k < max_pick; ++k) {
        const int klass = keys[k] == RCX_TPICK_NONE ? -1 : (int)keys[k];
        CHECK(klass == b.model0[k], "entry %llu: class %d, the model says %lld", (unsigned long long)k, klass, b.model0[k]);
    }
    // apply: the places and kept, for every entry of the tables
    std::vector<u64> ufirst(nent + 1, ~0ull), len_of(nent, 0), kept(max_pick, ~0ull);
    std::vector<u32> width_of(nent, 0), pred_of(nent, 0);
    std::vector<u8> placed(nent, 0);
    std::vector<long long> place_of(max_pick, -1);
    for (u64 t = 0; t < rcx_tpick_tiles(max_pick); ++t) {
        u64 before[NC] = {};
        for (u64 k = t * RCX_TPICK_THREADS; k < max_pick && k < (t + 1) * RCX_TPICK_THREADS; ++k) {
            const u32 key = k < count && !over ? keys[k] : RCX_TPICK_NONE;
            if (key == RCX_TPICK_NONE) {
                kept[k] = 0;
                continue;
            }
            const u64 place = (u64)cl.ent_first[key] + tile_ents.at(t * NC + key) + (before[key] >> RCX_TPICK_COUNT_SHIFT);
            CHECK(place < nent && !placed[place], "entry %llu: place %llu", (unsigned long long)k, (unsigned long long)place);
            placed[place] = 1;
            ufirst[place] = cl.ubase[key] + tile_units.at(t * NC + key) + (before[key] & LOW);
            len_of[place] = b.len[k];
            width_of[place] = b.widths[k];
            pred_of[place] = b.preds[k];
            place_of[k] = (long long)place;
            kept[k] = b.len[k];
            before[key] += sim_value(b.len[k], b.widths[k]);
        }
    }
    ufirst[nent] = cl.ubase[RCX_TYPED_CLASSES];
    for (u64 k = 0; k < max_pick; ++k) {
        CHECK(place_of[k] == b.model1[k], "entry %llu: place %lld, the model says %lld", (unsigned long long)k, place_of[k], b.model1[k]);
        CHECK(kept[k] == b.model2[k], "entry %llu: kept %llu, the model says %llu", (unsigned long long)k, (unsigned long long)kept[k], (unsigned long long)b.model2[k]);
    }
    if (over) {
        CHECK(nent == 0 && cl.step_end[RCX_TYPED_CLASSES - 1] == 0 && cl.rest_end[RCX_TYPED_CLASSES - 1] == 0, "an overflowing call has work");
        return true;
    }
    // the plan's invariants
    for (u32 k = 0; k < nent; ++k) {
        CHECK(placed[k], "place %u is empty", k);
        const u32 c = rcx_typed_class(width_of[k], pred_of[k]);
        CHECK(k >= cl.ent_first[c] && k < cl.ent_first[c + 1], "place %u is not in its class", k);
        CHECK(ufirst[k + 1] >= ufirst[k] && ufirst[k + 1] - ufirst[k] == rcx_tpick_units((u32)len_of[k], width_of[k]), "ufirst is not the prefix sum at %u", k);
    }
    // head, ufirst and rows against the host's plan of the same entries in the placed order
    {
        std::vector<u64> offs(nent + 1, 0), mem;
        std::vector<u8> w(nent + 1), pr(nent + 1);
        for (u32 k = 0; k < nent; ++k) offs[k + 1] = offs[k] + len_of[k], w[k] = (u8)width_of[k], pr[k] = (u8)pred_of[k];
        RcxTypedPlan p;
        CHECK(rcx_typed_plan(offs.data(), w.data(), pr.data(), nent, false, mem, p), "the host plan refuses the entries");
        const RcxTypedTables t = rcx_typed_tables(reinterpret_cast<const u8*>(mem.data()), p);
        CHECK(memcmp(t.classes, &cl, sizeof(cl)) == 0, "the head is not the host plan's");
        CHECK(p.nent == nent && p.nscan == 0 && memcmp(t.ufirst, ufirst.data(), (nent + 1) * sizeof(u64)) == 0, "ufirst is not the host plan's");
        for (u32 k = 0; k < nent; ++k) CHECK(t.len[k] == len_of[k], "place %u: %llu bytes, the host plan has %u", k, (unsigned long long)len_of[k], t.len[k]);
        const std::vector<u32> rowtab = sim_rows(cl, ufirst);
        const u32 rows = (u32)rowtab.size();
        const u64 bound = rcx_class_rows_most(b.max_bytes, RCX_TYPED_CLASSES);
        CHECK(rows == p.nrows && rows <= bound, "%u rows, bound %llu", rows, (unsigned long long)bound);
        for (u32 r = 0; r < rows; ++r) CHECK(rowtab[r] == t.rowtab[r], "row %u: entry %u, the host plan has %u", r, rowtab[r], t.rowtab[r]);
        if (!units_found(cl, ufirst, rowtab, which, "typed")) return false;
    }
    return true;
}

} // namespace

int main(int argc, char** argv) { return sim_typed_main<true>(argc, argv, "typed_split_picks_san", run); }
