// picks_san.hpp -- what the three sanitized rule programs of the class planner share (typed_picks_san.cpp, base_picks_san.cpp,
// typed_split_picks_san.cpp; cpprcoder_amd/csrc/rcx_class_plan.hpp): CHECK, the top step over the tile sums, a set's row table
// and the search of every unit.  Test tooling, not part of librcx.so.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cpprcoder_amd/csrc/rcx_base_picks.hpp"
#include "../../cpprcoder_amd/csrc/rcx_typed_split_picks.hpp"

uint64_t rcx_sim_counters[4];

#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("batch %d: ", which); \
            printf(__VA_ARGS__);         \
            printf("\n");                \
            return false;                \
        }                                \
    } while (0)

constexpr u64 SIM_LOW = (1ull << RCX_TPICK_COUNT_SHIFT) - 1ull;

// the value an entry gives to its key's sum
inline u64 sim_value(u64 len, u32 w) { return (1ull << RCX_TPICK_COUNT_SHIFT) | rcx_tpick_units((u32)len, w); }

// The top step: tile_sum[tiles][KEYS + 1] -> tile_ents, tile_units [tiles][KEYS], totals = the keys' entries, then their
// units; -> the bytes.
template <u32 KEYS>
u64 sim_top(const std::vector<u64>& tile_sum, std::vector<u32>& tile_ents, std::vector<u64>& tile_units, u64 (&totals)[2 * KEYS])
{
    const u64 tiles = tile_sum.size() / (KEYS + 1);
    tile_ents.assign(tiles * KEYS, 0), tile_units.assign(tiles * KEYS, 0);
    u64 bytes = 0;
    for (u32 c = 0; c < 2 * KEYS; ++c) totals[c] = 0;
    for (u64 t = 0; t < tiles; ++t) {
        for (u32 c = 0; c < KEYS; ++c) {
            const u64 v = tile_sum[t * (KEYS + 1) + c];
            tile_ents[t * KEYS + c] = (u32)totals[c];
            tile_units[t * KEYS + c] = totals[KEYS + c];
            totals[c] += v >> RCX_TPICK_COUNT_SHIFT;
            totals[KEYS + c] += v & SIM_LOW;
        }
        bytes += tile_sum[t * (KEYS + 1) + KEYS];
    }
    return bytes;
}

// a set's row table by the planner's rule
inline std::vector<u32> sim_rows(const RcxTypedClasses& cl, const std::vector<u64>& ufirst)
{
    std::vector<u32> rowtab(cl.row_first[RCX_TYPED_CLASSES]);
    for (u32 r = 0; r < rowtab.size(); ++r) rowtab[r] = rcx_class_row(cl, ufirst.data(), r);
    return rowtab;
}

// every unit of every class, searched between its row's bounds as the kernels search, lies in its own entry
inline bool units_found(const RcxTypedClasses& cl, const std::vector<u64>& ufirst, const std::vector<u32>& rowtab, int which, const char* name)
{
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c) {
        const u64 total = cl.ubase[c + 1] - cl.ubase[c];
        for (u64 u = 0; u < total; ++u) {
            const u64 g = cl.ubase[c] + u;
            const u32 row = cl.row_first[c] + (u32)(u / RCX_TYPED_ROW);
            const u32 k = rcx_typed_locate(ufirst.data(), rowtab.at(row), rowtab.at(row + 1), g);
            CHECK(k >= cl.ent_first[c] && k < cl.ent_first[c + 1] && ufirst[k] <= g && g < ufirst[k + 1], "%s set: unit %llu of class %u found in entry %u", name,
                  (unsigned long long)u, c, k);
        }
    }
    return true;
}

// The batches of the typed join's and the typed split's programs: per batch `n count max_bytes src_cap dst_cap status position`,
// then per entry `src_at dst_at len width pred` and two (EXTRA false) or three model columns.
struct TypedBatch {
    u64 count = 0, max_bytes = 0, src_cap = 0, dst_cap = 0;
    std::vector<u64> src_at, dst_at, len, model2;
    std::vector<u8> widths, preds;
    int status = 0;
    long long position = -1;
    std::vector<long long> model0, model1;
};

// -> the program's exit status
template <bool EXTRA, class Run>
int sim_typed_main(int argc, char** argv, const char* name, Run run)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int nbatches = 0;
    if (fscanf(f, "%d", &nbatches) != 1) return 2;
    u64 entries = 0;
    for (int i = 0; i < nbatches; ++i) {
        TypedBatch b;
        unsigned long long n, count, max_bytes, src_cap, dst_cap;
        if (fscanf(f, "%llu %llu %llu %llu %llu %d %lld", &n, &count, &max_bytes, &src_cap, &dst_cap, &b.status, &b.position) != 7) return 2;
        b.count = count, b.max_bytes = max_bytes, b.src_cap = src_cap, b.dst_cap = dst_cap;
        for (u64 k = 0; k < n; ++k) {
            unsigned long long a, d, len, m2 = 0;
            unsigned w, p;
            long long m0, m1;
            if (fscanf(f, "%llu %llu %llu %u %u %lld %lld", &a, &d, &len, &w, &p, &m0, &m1) != 7) return 2;
            if (EXTRA && fscanf(f, "%llu", &m2) != 1) return 2;
            b.src_at.push_back(a), b.dst_at.push_back(d), b.len.push_back(len), b.model2.push_back(m2);
            b.widths.push_back((u8)w), b.preds.push_back((u8)p);
            b.model0.push_back(m0), b.model1.push_back(m1);
        }
        if (!run(b, i)) return 1;
        entries += n;
    }
    fclose(f);
    printf("%s ok: %d batches, %llu entries\n", name, nbatches, (unsigned long long)entries);
    return 0;
}
