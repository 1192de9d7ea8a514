// base_picks_san.cpp -- the planner's rules of cpprcoder_amd/csrc/rcx_base_picks.hpp (rcx_bpick_validate, rcx_bpick_key,
// and, from rcx_typed_picks.hpp and the class planner, rcx_tpick_units, rcx_tpick_bin, rcx_class_head, rcx_class_row,
// rcx_class_rows_most: plain functions, the same text the kernels compile) in a program of its own, to be built with
// -fsanitize=address,undefined (tests/test_base_picks_cpu.py does).  It reads the batches base_items_cases.write_cases writes,
// plans each in the planner's steps -- keys and the 16 sums a tile, the sums over the tiles and both heads, the places, both
// row tables -- and checks
//   the host plan   rcx_base_items_plan of the same items in the same order: the head of both sets, ufirst exact, every
//                   position, length and base offset at its place, every row; the scan list holds the same items, in work order
//   the plan        every unit of every class of both sets, searched between its row's bounds as the kernels search, lies in
//                   its own entry; both row counts are within their bounds
// The tables lie in heap blocks of exactly their size, so a step outside is an error of the sanitizer as well.
// Test tooling, not part of librcx.so.
#include "picks_san.hpp"

namespace
{

struct Batch {
    std::vector<u64> offs{0}, boffs;
    std::vector<u8> widths, preds, ops;
    u64 first = 0, base_first = 0, base_bytes = 0;
};

struct Set {
    RcxTypedClasses cl;
    std::vector<u64> ufirst, from, bat;
    std::vector<u32> len, rowtab;
    std::vector<u8> placed;
};

bool run(const Batch& b, int which)
{
    const u64 n = b.widths.size(), count = n, tiles = rcx_tpick_tiles(count);
    const u64 bytes_all = b.offs[n] - b.offs[0], src_cap = b.offs[n], base_cap = b.base_first + b.base_bytes;
    // classify
    std::vector<u32> keys(n, RCX_TPICK_NONE), bins(RCX_TPICK_BINS, 0);
    constexpr u32 SUMS = RCX_BPICK_KEYS + 1u;
    std::vector<u64> tile_sum(tiles * SUMS, 0);
    for (u64 k = 0; k < count; ++k) {
        const u64 len = b.offs[k + 1] - b.offs[k];
        if (len == 0) continue;
        const u32 w = b.widths[k], pr = b.preds[k], op = b.ops[k];
        const u32 bad = rcx_bpick_validate(b.offs[k], b.offs[k], op != RCX_BASE_NONE_OP ? b.boffs[k] : 0, len, w, pr, op, src_cap, src_cap, base_cap);
        CHECK(bad == RCX_TPICK_OK, "entry %llu is refused with %u", (unsigned long long)k, bad);
        keys[k] = rcx_bpick_key((u32)len, w, pr, op);
        const u64 tile = k / RCX_TPICK_THREADS;
        if (keys[k] < RCX_BPICK_KEYS) tile_sum.at(tile * SUMS + keys[k]) += sim_value(len, w);
        else bins.at(keys[k] - RCX_BPICK_KEYS) += 1;
        tile_sum.at(tile * SUMS + RCX_BPICK_KEYS) += len;
    }
    // top
    std::vector<u64> tile_units;
    std::vector<u32> tile_ents;
    u64 totals[2 * RCX_BPICK_KEYS];
    const u64 bytes = sim_top<RCX_BPICK_KEYS>(tile_sum, tile_ents, tile_units, totals);
    CHECK(bytes == bytes_all, "%llu bytes of %llu", (unsigned long long)bytes, (unsigned long long)bytes_all);
    Set set[2];
    memset(&set[0].cl, 0, sizeof(RcxTypedClasses));
    memset(&set[1].cl, 0, sizeof(RcxTypedClasses));
    u64 of_class[2 * RCX_TYPED_CLASSES] = {}; // the typed set: key c = class 3 c
    for (u32 c = 0; c < RCX_BPICK_TYPED; ++c) of_class[3 * c] = totals[c], of_class[RCX_TYPED_CLASSES + 3 * c] = totals[RCX_BPICK_KEYS + c];
    rcx_class_head(of_class, of_class + RCX_TYPED_CLASSES, [](u32 w) { return rcx_base_items_rows(0u, w); }, set[0].cl);
    rcx_class_head(totals + RCX_BPICK_TYPED, totals + RCX_BPICK_KEYS + RCX_BPICK_TYPED, [](u32 w) { return rcx_base_items_rows(1u, w); }, set[1].cl);
    for (Set& s : set) {
        const u32 nent = s.cl.ent_first[RCX_TYPED_CLASSES];
        s.ufirst.assign(nent + 1, ~0ull), s.from.assign(nent, 0), s.bat.assign(nent, 0), s.len.assign(nent, 0), s.placed.assign(nent, 0);
        s.ufirst[nent] = s.cl.ubase[RCX_TYPED_CLASSES];
    }
    std::vector<u32> cursor(RCX_TPICK_BINS, 0);
    u32 nscan = 0;
    for (u32 i = 0; i < RCX_TPICK_BINS; ++i) {
        cursor[i] = nscan;
        nscan += bins[i];
    }
    // apply
    std::vector<u64> scan_from(nscan, 0);
    std::vector<u32> scan_len(nscan, 0);
    std::vector<u8> scan_kind(nscan, 0);
    for (u64 t = 0; t < tiles; ++t) {
        u64 before[RCX_BPICK_KEYS] = {};
        for (u64 k = t * RCX_TPICK_THREADS; k < count && k < (t + 1) * RCX_TPICK_THREADS; ++k) {
            const u32 key = keys[k];
            if (key == RCX_TPICK_NONE) continue;
            const u32 len = (u32)(b.offs[k + 1] - b.offs[k]), w = b.widths[k];
            if (key < RCX_BPICK_KEYS) {
                const bool based = key >= RCX_BPICK_TYPED;
                Set& s = set[based];
                const u32 c = based ? key - RCX_BPICK_TYPED : 3u * key;
                const u64 place = (u64)s.cl.ent_first[c] + tile_ents[t * RCX_BPICK_KEYS + key] + (before[key] >> RCX_TPICK_COUNT_SHIFT);
                CHECK(place < s.placed.size() && !s.placed[place], "entry %llu: place %llu", (unsigned long long)k, (unsigned long long)place);
                s.placed[place] = 1;
                s.ufirst[place] = s.cl.ubase[c] + tile_units[t * RCX_BPICK_KEYS + key] + (before[key] & SIM_LOW);
                s.from[place] = b.offs[k];
                s.bat[place] = based ? b.boffs[k] : 0;
                s.len[place] = len;
                before[key] += sim_value(len, w);
            } else {
                const u32 at = cursor.at(key - RCX_BPICK_KEYS)++;
                CHECK(at < nscan, "entry %llu: scan place %u of %u", (unsigned long long)k, at, nscan);
                scan_from[at] = b.offs[k], scan_len[at] = len, scan_kind[at] = (u8)(w | (b.preds[k] << 4));
            }
        }
    }
    // rows
    const u64 bound[2] = {rcx_class_rows_most(bytes, RCX_BPICK_TYPED), rcx_class_rows_most(bytes, RCX_TYPED_CLASSES)};
    for (u32 i = 0; i < 2; ++i) {
        Set& s = set[i];
        s.rowtab = sim_rows(s.cl, s.ufirst);
        CHECK(s.rowtab.size() <= bound[i], "set %u: %llu rows, bound %llu", i, (unsigned long long)s.rowtab.size(), (unsigned long long)bound[i]);
        for (u8 p : s.placed) CHECK(p, "set %u: a place is empty", i);
    }
    // the host plan of the same items in the same order
    std::vector<u64> mem;
    RcxBaseItemsPlan p;
    CHECK(rcx_base_items_plan(b.offs.data(), b.boffs.data(), b.widths.data(), b.preds.data(), b.ops.data(), n, true, mem, p), "the host plan refuses the items");
    const u8* const h = reinterpret_cast<const u8*>(mem.data());
    const RcxTypedTables tt = rcx_typed_tables(h, p.typed);
    const RcxBaseItemsTables bt = rcx_base_items_tables(h, p);
    const RcxTypedTables* const theirs[2] = {&tt, &bt.t};
    const RcxTypedPlan* const plans[2] = {&p.typed, &p.based};
    for (u32 i = 0; i < 2; ++i) {
        const Set& s = set[i];
        const RcxTypedTables& t = *theirs[i];
        const u64 nent = s.from.size();
        CHECK(memcmp(t.classes, &s.cl, sizeof(s.cl)) == 0, "set %u: the head is not the host plan's", i);
        CHECK(plans[i]->nent == nent && plans[i]->nrows == s.rowtab.size(), "set %u: %llu entries and %llu rows, the host plan has %llu and %llu", i,
              (unsigned long long)nent, (unsigned long long)s.rowtab.size(), (unsigned long long)plans[i]->nent, (unsigned long long)plans[i]->nrows);
        CHECK(memcmp(t.ufirst, s.ufirst.data(), (nent + 1) * sizeof(u64)) == 0, "set %u: ufirst is not the host plan's", i);
        for (u64 k = 0; k < nent; ++k) {
            CHECK(t.at[k] == s.from[k] && t.len[k] == s.len[k], "set %u: place %llu holds another entry than the host plan's", i, (unsigned long long)k);
            if (i) CHECK(bt.bat[k] == s.bat[k], "place %llu: base offset %llu, the host plan has %llu", (unsigned long long)k, (unsigned long long)s.bat[k],
                         (unsigned long long)bt.bat[k]);
        }
        for (u64 r = 0; r < s.rowtab.size(); ++r) CHECK(t.rowtab[r] == s.rowtab[r], "set %u row %llu: entry %u, the host plan has %u", i, (unsigned long long)r, s.rowtab[r], t.rowtab[r]);
        if (!units_found(s.cl, s.ufirst, s.rowtab, which, i ? "base" : "typed")) return false;
    }
    // the scan list: the host plan's items, in work order (ascending bins = descending lengths)
    CHECK(nscan == tt.nscan, "%u scan entries, the host plan has %llu", nscan, (unsigned long long)tt.nscan);
    std::vector<u64> mine, host;
    for (u32 s = 0; s < nscan; ++s) {
        CHECK(scan_len[s] > 0, "scan place %u is empty", s);
        if (s + 1 < nscan) CHECK(rcx_tpick_bin(scan_len[s]) <= rcx_tpick_bin(scan_len[s + 1]), "the scan list is out of order at %u", s);
        mine.push_back(scan_from[s] ^ ((u64)scan_len[s] << 40) ^ ((u64)scan_kind[s] << 32));
        host.push_back(tt.scan_at[s] ^ ((u64)tt.scan_len[s] << 40) ^ ((u64)tt.scan_kind[s] << 32));
    }
    std::sort(mine.begin(), mine.end());
    std::sort(host.begin(), host.end());
    CHECK(mine == host, "the scan list holds other items than the host plan's");
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned count = 0;
    if (fscanf(f, "%u", &count) != 1) return 2;
    unsigned long long items = 0;
    for (unsigned k = 0; k < count; ++k) {
        unsigned long long n = 0, first = 0, bfirst = 0, bbytes = 0;
        if (fscanf(f, "%llu %llu %llu %llu", &n, &first, &bfirst, &bbytes) != 4) return 2;
        Batch b;
        b.offs[0] = first;
        b.first = first, b.base_first = bfirst, b.base_bytes = bbytes;
        for (unsigned long long i = 0; i < n; ++i) {
            unsigned long long len = 0, boff = 0;
            unsigned w = 0, pr = 0, op = 0;
            if (fscanf(f, "%llu %u %u %u %llu", &len, &w, &pr, &op, &boff) != 5) return 2;
            b.offs.push_back(b.offs.back() + len);
            b.boffs.push_back(boff);
            b.widths.push_back((u8)w), b.preds.push_back((u8)pr), b.ops.push_back((u8)op);
        }
        if (!run(b, (int)k)) return 1;
        items += n;
    }
    fclose(f);
    printf("base_picks_san ok: %u batches, %llu entries\n", count, items);
    return 0;
}
