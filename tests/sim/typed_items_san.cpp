// typed_items_san.cpp -- the plan and the mapping of cpprcoder_amd/csrc/rcx_typed_items.hpp (rcx_typed_plan, rcx_typed_class_of,
// rcx_typed_locate over rcx_typed_locate_step, rcx_typed_rest_of: plain functions, the same text the kernels compile) in a program of its own, to be
// built with -fsanitize=address,undefined (tests/test_typed_items_cpu.py does).  It reads batches of typed items from a
// file, plans each for split and for join, and walks the plan as the kernels do -- a grid of a few workgroups that loops
// over the steps and the rest blocks, every lane of every row; a wave an item of the scan list -- counting for every byte of
// the batch how often it is read and how often it is written.  Every byte of every item must come out exactly once on
// both sides, and nothing else may be touched: the counters cover exactly the batch's bytes, and the tables lie in heap
// blocks of exactly their size, so a step outside either is an error of the sanitizer as well.
// Test tooling, not part of librcx.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cpprcoder_amd/csrc/rcx_typed_items.hpp"

uint64_t rcx_sim_counters[4];

namespace
{

struct Batch {
    std::vector<u64> offs;
    std::vector<u8> widths, preds;
};

struct Counts {
    u64 base, n;
    std::vector<u8> reads, writes;
    bool ok = true;
    void touch(std::vector<u8>& c, u64 at, u64 bytes, const char* what)
    {
        if (at < base || at + bytes > base + n) {
            printf("%s outside the batch: %llu + %llu\n", what, (unsigned long long)at, (unsigned long long)bytes);
            ok = false;
            return;
        }
        for (u64 i = 0; i < bytes; ++i) c.at(at - base + i) += 1;
    }
    void read(u64 at, u64 bytes) { touch(reads, at, bytes, "read"); }
    void write(u64 at, u64 bytes) { touch(writes, at, bytes, "write"); }
};

// one unit of entry (at, m) of width W: 16 W bytes of elements, 16 bytes of each plane
void unit(Counts& c, bool join, u32 W, u64 at, u32 m, u32 u)
{
    const u64 elements = at + (u64)u * (16u * W), planes = at + 16ull * u;
    join ? c.write(elements, 16u * W) : c.read(elements, 16u * W);
    for (u32 p = 0; p < W; ++p) join ? c.read(planes + (u64)p * m, 16) : c.write(planes + (u64)p * m, 16);
}

template <u32 W>
void rest_lane(Counts& c, bool join, const RcxTypedTables& t, u32 first, u32 count, u64 r)
{
    const u64 k = r / (17u * W);
    if (k >= count) return;
    const u32 j = (u32)(r - k * (17u * W)), len = t.len[first + k], m = len / W;
    const u64 at = t.at[first + k];
    u32 e, p;
    const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
    if (kind == 1) {
        const u64 element = at + (u64)e * W + p, plane = at + (u64)p * m + e;
        c.read(join ? plane : element, 1);
        c.write(join ? element : plane, 1);
    } else if (kind == 2) {
        c.read(at + e, 1);
        c.write(at + e, 1);
    }
}

// rcx_typed_items_k with `grid` workgroups
void rows_kernel(Counts& c, bool join, const RcxTypedTables& t, u32 grid)
{
    const RcxTypedClasses* cl = t.classes;
    for (u32 block = 0; block < grid; ++block) {
        for (u64 s = block; s < cl->step_end[RCX_TYPED_CLASSES - 1]; s += grid) {
            const u32 cls = rcx_typed_class_of(cl->step_end, s), W = rcx_typed_class_width(cls), K = RCX_PLANES_U4 / W;
            const u64 local = s - (cls ? cl->step_end[cls - 1] : 0), ubase = cl->ubase[cls], total = cl->ubase[cls + 1] - ubase;
            const u64 base = local * K * RCX_TYPED_ROW;
            const u32 row0 = cl->row_first[cls] + (u32)(local * K);
            for (u32 j = 0; j < K; ++j) {
                const u64 first = base + (u64)j * RCX_TYPED_ROW;
                if (first >= total) continue;
                for (u32 tid = 0; tid < RCX_TYPED_ROW; ++tid) {
                    const bool live = first + tid < total;
                    const u64 g = ubase + (live ? first + tid : total - 1);
                    const u32 k = rcx_typed_locate(t.ufirst, t.rowtab[row0 + j], t.rowtab[row0 + j + 1], g);
                    const u32 m = t.len[k] / W, u = (u32)(g - t.ufirst[k]);
                    if (k < cl->ent_first[cls] || k >= cl->ent_first[cls + 1] || u >= (m >> 4)) {
                        printf("unit %llu of class %u: entry %u unit %u\n", (unsigned long long)(first + tid), cls, k, u);
                        c.ok = false;
                        continue;
                    }
                    if (live) unit(c, join, W, t.at[k], m, u);
                }
            }
        }
        for (u64 b = block; b < cl->rest_end[RCX_TYPED_CLASSES - 1]; b += grid) {
            const u32 cls = rcx_typed_class_of(cl->rest_end, b), W = rcx_typed_class_width(cls);
            const u32 first = cl->ent_first[cls], count = cl->ent_first[cls + 1] - first;
            for (u32 tid = 0; tid < RCX_TYPED_ROW; ++tid) {
                const u64 r = (b - (cls ? cl->rest_end[cls - 1] : 0)) * RCX_TYPED_ROW + tid;
                if (W == 1) rest_lane<1>(c, join, t, first, count, r);
                else if (W == 2) rest_lane<2>(c, join, t, first, count, r);
                else if (W == 4) rest_lane<4>(c, join, t, first, count, r);
                else rest_lane<8>(c, join, t, first, count, r);
            }
        }
    }
}

// rcx_typed_items_scan_k: a wave an item, tile by tile; then the last m % 16 elements, then the tail
bool scan_kernel(Counts& c, const RcxTypedTables& t, u32 grid)
{
    u32 before = 0xFFFFFFFFu;
    for (u32 block = 0; block < grid; ++block)
        for (u64 i = block; i < t.nscan; i += grid) {
            const u64 at = t.scan_at[i];
            const u32 len = t.scan_len[i], W = t.scan_kind[i] & 15u, pred = t.scan_kind[i] >> 4;
            if (!(W == 2 || W == 4 || W == 8) || !(pred == 1 || pred == 2) || len == 0) return false;
            const u32 m = len / W, units = m >> 4, rows = (units + 63) / 64;
            for (u32 row = 0; row < rows; ++row)
                for (u32 lane = 0; lane < 64; ++lane)
                    if (row * 64 + lane < units) unit(c, true, W, at, m, row * 64 + lane);
            for (u32 lane = 0; lane < m - (m & ~15u); ++lane) {
                for (u32 p = 0; p < W; ++p) c.read(at + (u64)p * m + (m & ~15u) + lane, 1);
                c.write(at + (u64)((m & ~15u) + lane) * W, W);
            }
            for (u32 lane = 0; lane < len - m * W; ++lane) {
                c.read(at + (u64)m * W + lane, 1);
                c.write(at + (u64)m * W + lane, 1);
            }
        }
    for (u64 i = 0; i < t.nscan; ++i) { // longest first
        if (t.scan_len[i] > before) return false;
        before = t.scan_len[i];
    }
    return true;
}

bool run(const Batch& b, bool join, u32 grid, u32 which)
{
    const u64 nitems = b.widths.size();
    std::vector<u64> mem;
    RcxTypedPlan p;
    if (!rcx_typed_plan(b.offs.data(), b.widths.data(), b.preds.data(), nitems, join, mem, p)) return false;
    u8* tables = static_cast<u8*>(malloc(p.bytes)); // exactly the tables: a read past them is the sanitizer's to report
    memcpy(tables, mem.data(), p.bytes);
    const RcxTypedTables t = rcx_typed_tables(tables, p);
    Counts c;
    c.base = b.offs[0];
    c.n = b.offs[nitems] - b.offs[0];
    c.reads.assign(c.n, 0);
    c.writes.assign(c.n, 0);
    rows_kernel(c, join, t, grid);
    if (!scan_kernel(c, t, grid + 1)) c.ok = false;
    if (!join && p.nscan) c.ok = false;
    for (u64 i = 0; i < c.n && c.ok; ++i)
        if (c.reads[i] != 1 || c.writes[i] != 1) {
            printf("batch %u %s: byte %llu read %u times, written %u times\n", which, join ? "join" : "split", (unsigned long long)i, c.reads[i], c.writes[i]);
            c.ok = false;
        }
    free(tables);
    return c.ok;
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
        unsigned long long n = 0, base = 0;
        if (fscanf(f, "%llu %llu", &n, &base) != 2) return 2;
        Batch b;
        b.offs.push_back(base);
        for (unsigned long long i = 0; i < n; ++i) {
            unsigned long long len = 0;
            unsigned w = 0, pr = 0;
            if (fscanf(f, "%llu %u %u", &len, &w, &pr) != 3) return 2;
            b.offs.push_back(b.offs.back() + len);
            b.widths.push_back((u8)w);
            b.preds.push_back((u8)pr);
        }
        items += n;
        for (u32 grid : {1u, 3u, 1024u})
            for (int join = 0; join < 2; ++join)
                if (!run(b, join != 0, grid, k)) {
                    printf("batch %u failed (grid %u, %s)\n", k, grid, join ? "join" : "split");
                    return 1;
                }
    }
    fclose(f);
    printf("typed_items_san ok: %u batches, %llu items\n", count, items);
    return 0;
}
