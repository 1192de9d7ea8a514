// base_items_san.cpp -- the plan and the mapping of cpprcoder_amd/csrc/rcx_base_items.hpp (rcx_base_items_plan over the mapping
// functions of rcx_typed_items.hpp: plain functions, the same text the kernels compile) in a program of its own, to be built
// with -fsanitize=address,undefined (tests/test_base_items_cpu.py does).  It reads batches of items from a file, plans each
// for split and for join, and walks both sets of tables as the kernels do -- a grid of a few workgroups that loops over
// the steps and the rest blocks, every lane of every row, with rcx_typed_step's rows for the items without an op and
// rcx_base_items_step's for those with one; a wave an item of the scan list -- counting for every byte of the batch how often
// it is read and how often it is written.  Every byte of every item must come out exactly once on both sides, nothing else
// may be touched, every read of the base must lie inside the span of the item it serves, and every entry of the base set
// must be an item of the batch with its own span.  Where no item has an op the typed set must equal rcx_typed_plan's byte
// for byte.  The tables lie in heap blocks of exactly their size, so a step outside is an error of the sanitizer as well.
// Test tooling, not part of librcx.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "../../cpprcoder_amd/csrc/rcx_base_items.hpp"

uint64_t rcx_sim_counters[4];

namespace
{

struct Batch {
    std::vector<u64> offs, boffs;
    std::vector<u8> widths, preds, ops;
    u64 base_first = 0, base_bytes = 0;
    bool any_op = false;
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

struct Walk {
    Counts c;
    const Batch* b;
    bool join;
    const u64* bat; // the base set's, nullptr while the typed set is walked
    u64 base_reads = 0;
    // a read of the base for entry k: inside the whole elements of its span, inside the base
    void theirs(const RcxTypedTables& t, u32 k, u32 W, u64 at, u64 bytes)
    {
        const u64 span = bat[k], whole = (u64)(t.len[k] / W) * W;
        if (at < span || at + bytes > span + whole || at < b->base_first || at + bytes > b->base_first + b->base_bytes) {
            printf("base read outside: entry %u, %llu + %llu\n", k, (unsigned long long)at, (unsigned long long)bytes);
            c.ok = false;
        }
        base_reads += bytes;
    }
};

// one unit of entry k of width W: 16 W bytes of elements, 16 bytes of each plane, and with a base 16 W bytes of it
void unit(Walk& wk, const RcxTypedTables& t, u32 W, u32 k, u32 u)
{
    const u64 at = t.at[k];
    const u32 m = t.len[k] / W;
    const u64 elements = at + (u64)u * (16u * W), planes = at + 16ull * u;
    wk.join ? wk.c.write(elements, 16u * W) : wk.c.read(elements, 16u * W);
    for (u32 p = 0; p < W; ++p) wk.join ? wk.c.read(planes + (u64)p * m, 16) : wk.c.write(planes + (u64)p * m, 16);
    if (wk.bat) wk.theirs(t, k, W, wk.bat[k] + (u64)u * (16u * W), 16u * W);
}

template <u32 W>
void rest_lane(Walk& wk, const RcxTypedTables& t, u32 first, u32 count, u64 r)
{
    const u64 k = r / (17u * W);
    if (k >= count) return;
    const u32 j = (u32)(r - k * (17u * W)), len = t.len[first + k], m = len / W;
    const u64 at = t.at[first + k];
    u32 e, p;
    const u32 kind = rcx_typed_rest_of<W>(len, j, e, p);
    if (kind == 1) {
        const u64 element = at + (u64)e * W + p, plane = at + (u64)p * m + e;
        wk.c.read(wk.join ? plane : element, 1); // (with a base the lane reads the whole element; its own byte is what counts)
        wk.c.write(wk.join ? element : plane, 1);
        if (wk.bat && p == 0) wk.theirs(t, (u32)(first + k), W, wk.bat[first + k] + (u64)e * W, W);
    } else if (kind == 2) {
        wk.c.read(at + e, 1);
        wk.c.write(at + e, 1);
    }
}

// rcx_typed_items_k (set 0) or rcx_base_items_k (set 1) with `grid` workgroups
void rows_kernel(Walk& wk, const RcxTypedTables& t, u32 set, u32 grid)
{
    const RcxTypedClasses* cl = t.classes;
    Counts& c = wk.c;
    for (u32 block = 0; block < grid; ++block) {
        for (u64 s = block; s < cl->step_end[RCX_TYPED_CLASSES - 1]; s += grid) {
            const u32 cls = rcx_typed_class_of(cl->step_end, s), W = rcx_typed_class_width(cls), K = rcx_base_items_rows(set, W);
            const u64 local = s - (cls ? cl->step_end[cls - 1] : 0), ubase = cl->ubase[cls], total = cl->ubase[cls + 1] - ubase;
            const u64 base = local * K * RCX_TYPED_ROW;
            const u32 row0 = cl->row_first[cls] + (u32)(local * K);
            if (base >= total) {
                printf("step %llu of class %u has no unit\n", (unsigned long long)local, cls);
                c.ok = false;
            }
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
                    if (live) unit(wk, t, W, k, u);
                }
            }
        }
        for (u64 b = block; b < cl->rest_end[RCX_TYPED_CLASSES - 1]; b += grid) {
            const u32 cls = rcx_typed_class_of(cl->rest_end, b), W = rcx_typed_class_width(cls);
            const u32 first = cl->ent_first[cls], count = cl->ent_first[cls + 1] - first;
            for (u32 tid = 0; tid < RCX_TYPED_ROW; ++tid) {
                const u64 r = (b - (cls ? cl->rest_end[cls - 1] : 0)) * RCX_TYPED_ROW + tid;
                if (W == 1) rest_lane<1>(wk, t, first, count, r);
                else if (W == 2) rest_lane<2>(wk, t, first, count, r);
                else if (W == 4) rest_lane<4>(wk, t, first, count, r);
                else rest_lane<8>(wk, t, first, count, r);
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
            const u32 m = len / W, units = m >> 4;
            for (u32 u = 0; u < units; ++u) {
                c.write(at + (u64)u * (16u * W), 16u * W);
                for (u32 p = 0; p < W; ++p) c.read(at + 16ull * u + (u64)p * m, 16);
            }
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

// every entry of the base set is an item of the batch with an op: its class, its bytes, its own span; and every such item is there
bool entries_match(const Batch& b, const RcxBaseItemsTables& bt, const RcxBaseItemsPlan& p)
{
    std::map<u64, u64> item_at;
    u64 want = 0, whole = 0;
    for (u64 i = 0; i < b.widths.size(); ++i)
        if (b.ops[i] != RCX_BASE_NONE_OP && b.offs[i + 1] > b.offs[i]) item_at[b.offs[i]] = i, ++want;
    if (want != p.based.nent) return false;
    const RcxTypedClasses* cl = bt.t.classes;
    for (u32 c = 0; c < RCX_TYPED_CLASSES; ++c)
        for (u32 k = cl->ent_first[c]; k < cl->ent_first[c + 1]; ++k) {
            const auto it = item_at.find(bt.t.at[k]);
            if (it == item_at.end()) return false;
            const u64 i = it->second;
            if (rcx_typed_class(b.widths[i], b.ops[i]) != c || bt.t.len[k] != b.offs[i + 1] - b.offs[i] || bt.bat[k] != b.boffs[i]) return false;
            whole += (u64)(bt.t.len[k] / b.widths[i]) * b.widths[i];
            item_at.erase(it);
        }
    rcx_sim_counters[0] = whole;
    return item_at.empty();
}

bool run(const Batch& b, bool join, u32 grid, u32 which)
{
    const u64 nitems = b.widths.size();
    std::vector<u64> mem;
    RcxBaseItemsPlan p;
    if (!rcx_base_items_plan(b.offs.data(), b.boffs.data(), b.widths.data(), b.preds.data(), b.ops.data(), nitems, join, mem, p)) return false;
    u8* tables = static_cast<u8*>(malloc(p.bytes)); // exactly the tables: a read past them is the sanitizer's to report
    memcpy(tables, mem.data(), p.bytes);
    const RcxTypedTables t = rcx_typed_tables(tables, p.typed);
    const RcxBaseItemsTables bt = rcx_base_items_tables(tables, p);
    Walk wk;
    wk.b = &b;
    wk.join = join;
    Counts& c = wk.c;
    c.base = b.offs[0];
    c.n = b.offs[nitems] - b.offs[0];
    c.reads.assign(c.n, 0);
    c.writes.assign(c.n, 0);
    if (!b.any_op) { // rcx_typed_plan's tables, byte for byte, and nothing for the other kernel
        std::vector<u64> theirs;
        RcxTypedPlan q;
        if (!rcx_typed_plan(b.offs.data(), b.widths.data(), b.preds.data(), nitems, join, theirs, q)) return false;
        if (q.bytes != p.typed.bytes || memcmp(theirs.data(), tables, q.bytes) != 0 || q.o_ufirst != p.typed.o_ufirst || q.o_at != p.typed.o_at
            || q.o_scan_at != p.typed.o_scan_at || q.o_len != p.typed.o_len || q.o_rowtab != p.typed.o_rowtab || q.o_scan_len != p.typed.o_scan_len
            || q.o_scan_kind != p.typed.o_scan_kind || q.nent != p.typed.nent || q.nrows != p.typed.nrows || q.nscan != p.typed.nscan
            || q.steps != p.typed.steps || q.rest_blocks != p.typed.rest_blocks || p.based.steps || p.based.rest_blocks || p.based.nent) {
            printf("batch %u %s: the typed set is not rcx_typed_plan's\n", which, join ? "join" : "split");
            c.ok = false;
        }
        // the same plan from a batch whose ops say "none" one by one, and from one that has no table of ops
        std::vector<u64> again;
        RcxBaseItemsPlan p2;
        if (!rcx_base_items_plan(b.offs.data(), nullptr, b.widths.data(), b.preds.data(), nullptr, nitems, join, again, p2) || p2.bytes != p.bytes
            || memcmp(again.data(), tables, p.bytes) != 0)
            c.ok = false;
    }
    wk.bat = nullptr;
    rows_kernel(wk, t, 0, grid);
    if (!scan_kernel(c, t, grid + 1)) c.ok = false;
    if (!join && p.typed.nscan) c.ok = false;
    if (!entries_match(b, bt, p)) {
        printf("batch %u %s: the base set's entries are not the batch's items with an op\n", which, join ? "join" : "split");
        c.ok = false;
    }
    wk.bat = bt.bat;
    rows_kernel(wk, bt.t, 1, grid);
    if (wk.base_reads != rcx_sim_counters[0]) { // every whole element of every span in use, once
        printf("batch %u %s: %llu bytes of the base read, %llu expected\n", which, join ? "join" : "split", (unsigned long long)wk.base_reads,
               (unsigned long long)rcx_sim_counters[0]);
        c.ok = false;
    }
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
        unsigned long long n = 0, first = 0, bfirst = 0, bbytes = 0;
        if (fscanf(f, "%llu %llu %llu %llu", &n, &first, &bfirst, &bbytes) != 4) return 2;
        Batch b;
        b.base_first = bfirst;
        b.base_bytes = bbytes;
        b.offs.push_back(first);
        for (unsigned long long i = 0; i < n; ++i) {
            unsigned long long len = 0, boff = 0;
            unsigned w = 0, pr = 0, op = 0;
            if (fscanf(f, "%llu %u %u %u %llu", &len, &w, &pr, &op, &boff) != 5) return 2;
            b.offs.push_back(b.offs.back() + len);
            b.boffs.push_back(boff);
            b.widths.push_back((u8)w);
            b.preds.push_back((u8)pr);
            b.ops.push_back((u8)op);
            if (op != RCX_BASE_NONE_OP) b.any_op = true;
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
    printf("base_items_san ok: %u batches, %llu items\n", count, items);
    return 0;
}
