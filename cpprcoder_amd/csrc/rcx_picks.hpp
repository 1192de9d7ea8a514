// rcx_picks.hpp -- the planner of rcx_decode_picks_device (include/rcx_picks.h): what plan_items and plan_stored_picks do on
// the host (rcx_items.hpp, rcx_stored_api.hpp) for tables that are in device memory.  Four kernels, one launch each:
//
//   rcx_picks_clear_k      bins[] = 0 (the table scratch holds another call's tables when this one starts).  A kernel, not
//                          hipMemsetAsync: captured in a graph, the memset did its work in the first replay only and the
//                          counts of the replays added up; a captured call is kernel nodes alone.
//   rcx_picks_classify_k   entry k < min(*d_count, max_pick): validate it (the rules of the header, in their order) and give
//                          it a BIN -- its place in the work order up to the order inside a bin -- or none; bins[] counts the
//                          entries of every bin.  keys[k] = the bin, RCX_PICK_NONE for an entry that is skipped.
//   rcx_picks_scan_k       one workgroup: cursor[b] = the entries of the bins before b, counts[] = {coded, stored long, stored
//                          short} entries.
//   rcx_picks_scatter_k    entry k with a bin takes the next place of its bin and writes {at, len, id, stream} there.
//
// The work order is a counting sort, not a sort: a wave runs as long as its longest entry, so it should carry entries of
// similar length, and the long chains should start first -- which asks for nothing about entries of (nearly) one length.
// The bins, in work order:
//   coded picks, longest first   a length below 512 has a bin of its own; above, the bin is the length's leading one and the
//                                eight bits behind it, so the lengths of a bin differ by less than 1/256 (RCX_PICK_CODED_BINS
//                                bins: RCX_MAX_BLOCK is below 2^24)
//   stored picks above RCX_COPY_SHORT bytes, then the other stored picks: the two kinds of entry of the copy kernel, which
//                                is bound by bandwidth, not by its longest entry: no order inside either
// Which place of its bin an entry gets depends on which wave asks first, so the order inside a bin changes from call to
// call; no output depends on it (every entry has its own destination, and a failure is reported by pick position).
//
// The counters are taken a wave at a time: the lanes of a wave that want the same bin send one atomic between them.  With
// picks of one length -- pages -- that is one atomic a wave and not 64 to one address.
// No LDS apart from the scan's, no inline assembly, no scratch; nothing is read behind min(*d_count, max_pick).
#pragma once
#include "rcx_lane.hpp"

#define RCX_PICK_EXACT 512u                                          // lengths below this have a bin each
#define RCX_LEN_BINS(top_bits) (RCX_PICK_EXACT + ((top_bits) - 9u) * 256u) // the bins of the lengths below 2^top_bits
#define RCX_PICK_CODED_BINS RCX_LEN_BINS(24u)                        // 4352
#define RCX_PICK_BINS (RCX_PICK_CODED_BINS + 2u)                     // + stored long, stored short
#define RCX_PICK_NONE 0xFFFFFFFFu
#define RCX_PICK_THREADS 256
#define RCX_PICK_SCAN_THREADS 1024

// the bin of `len` bytes, 1 <= len < 2^top_bits, among RCX_LEN_BINS(top_bits): ascending bins = descending length.  The one
// rule of every work order here: rcx_pick_bin, rcx_epick_bin (rcx_encode_picks.hpp), rcx_tpick_bin (rcx_typed_picks.hpp).
RCX_HD u32 rcx_len_bin(u32 len, u32 top_bits)
{
    u32 up = len;
    if (len >= RCX_PICK_EXACT) {
        u32 e = 9;
        while ((len >> e) > 1u) ++e; // the leading one, 9 .. top_bits - 1
        up = RCX_PICK_EXACT + (e - 9u) * 256u + ((len >> (e - 8u)) & 255u);
    }
    return RCX_LEN_BINS(top_bits) - 1u - up;
}

// the bin of a coded pick of `len` bytes, 1 <= len < 2^24
RCX_HD u32 rcx_pick_bin(u32 len) { return rcx_len_bin(len, 24u); }

#if !defined(RCX_HOST_SIM)

#include <hip/hip_runtime.h>

#include "rcx_predict.hpp" // rcx_wave_scan
#include "rcx_stored.hpp"

// What the call is given, as the kernels take it.
struct RcxPickTables {
    const u64* pick;
    const u64* dst_at;
    const u64* dst_len;
    const u64* count;
    const u8* stored; // or nullptr
    const u64* comp_offsets;
    u64 comp_size, nstreams, max_pick, dst_cap;
    u32 max_len;
};

// The planned tables (RcxItems without `inv`) and the planner's own words, all in the context's table scratch.
struct RcxPickPlan {
    u64* at;
    u32* len;
    u32* id;
    u32* stream;
    u32* keys;   // [max_pick]
    u32* cursor; // [RCX_PICK_BINS]
    u32* bins;   // [RCX_PICK_BINS], zero when the classify kernel starts
    u32* counts; // [4]: coded, stored long, stored short entries
};

// `has` lanes add 1 to counters[bin]; -> what the lane's own 1 found there.  Every lane of the wave calls it.
__device__ __forceinline__ u32 rcx_pick_take(u32* counters, u32 bin, bool has)
{
    const u32 lane = threadIdx.x & 63u;
    u32 place = 0;
    u64 todo = __ballot(has);
    while (todo) { // (the same in every lane)
        const int first = __ffsll((unsigned long long)todo) - 1;
        const u32 b = (u32)__shfl((int)bin, first, 64);
        const bool mine = has && bin == b;
        const u64 same = __ballot(mine);
        u32 base = 0;
        if (lane == (u32)first) base = atomicAdd(&counters[b], (u32)__popcll(same));
        base = (u32)__shfl((int)base, first, 64);
        if (mine) place = base + (u32)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return place;
}

// how many of the `most` entries are meant
__device__ __forceinline__ u64 rcx_pick_count(const u64* count, u64 most)
{
    const u64 c = count[0];
    return c < most ? c : most;
}

// Inclusive sums over the RCX_PICK_SCAN_THREADS threads of the one workgroup; all = the workgroup's total.  lds: 16 words; in
// step at its end.
template <class T>
__device__ __forceinline__ T rcx_group_scan(T x, T* lds, T& all)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T upto = rcx_wave_scan<T>(x, lane);
    if (lane == 63u) lds[wave] = upto;
    __syncthreads();
    T front = 0;
    all = 0;
#pragma unroll
    for (u32 w = 0; w < RCX_PICK_SCAN_THREADS / 64u; ++w) {
        const T v = lds[w];
        front += w < wave ? v : (T)0;
        all += v;
    }
    __syncthreads();
    return upto + front;
}

// The exclusive sum of bins[BINS] by the one workgroup: each(b, before, mine) for every bin b, before = the entries of the
// bins in front of it, mine = its own; -> the entries of all bins.  lds: 16 words.
template <u32 BINS, class F>
__device__ __forceinline__ u32 rcx_bins_scan(const u32* bins, u32* lds, F&& each)
{
    constexpr u32 PER = (BINS + RCX_PICK_SCAN_THREADS - 1) / RCX_PICK_SCAN_THREADS;
    const u32 b0 = threadIdx.x * PER;
    u32 mine[PER], sum = 0;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        mine[j] = b0 + j < BINS ? bins[b0 + j] : 0u;
        sum += mine[j];
    }
    u32 all;
    u32 before = rcx_group_scan<u32>(sum, lds, all) - sum;
#pragma unroll
    for (u32 j = 0; j < PER; ++j) {
        if (b0 + j < BINS) each(b0 + j, before, mine[j]);
        before += mine[j];
    }
    return all;
}

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_picks_clear_k(const RcxPickPlan p)
{
    const u32 b = blockIdx.x * RCX_PICK_THREADS + threadIdx.x;
    if (b < RCX_PICK_BINS) p.bins[b] = 0;
}

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_picks_classify_k(const RcxPickTables t, const RcxPickPlan p, u32* status)
{
    const u64 count = rcx_pick_count(t.count, t.max_pick);
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.count[0] > t.max_pick) rcx_flag(status, RCX_ST_CAPACITY, t.max_pick);
    // whole waves: every lane of a wave that has an entry goes round
    for (u64 k0 = (u64)blockIdx.x * RCX_PICK_THREADS; k0 < count; k0 += (u64)gridDim.x * RCX_PICK_THREADS) {
        const u64 k = k0 + threadIdx.x;
        u32 bin = RCX_PICK_NONE;
        if (k < count) {
            const u64 len = t.dst_len[k];
            if (len != 0) { // (a length of 0 is not looked at)
                const u64 st = t.pick[k], at = t.dst_at[k];
                if (st >= t.nstreams || len > (u64)t.max_len) {
                    rcx_flag(status, RCX_ST_CORRUPT, k);
                } else if (at > t.dst_cap || len > t.dst_cap - at) {
                    rcx_flag(status, RCX_ST_CAPACITY, k);
                } else if (t.stored && t.stored[st]) {
                    const u64 s0 = t.comp_offsets[st], s1 = t.comp_offsets[st + 1];
                    if (s1 >= s0 && s1 <= t.comp_size && s1 - s0 == len) bin = RCX_PICK_CODED_BINS + (len > RCX_COPY_SHORT ? 0u : 1u);
                    else rcx_flag(status, RCX_ST_CORRUPT, k);
                } else {
                    bin = rcx_pick_bin((u32)len);
                }
            }
            p.keys[k] = bin;
        }
        (void)rcx_pick_take(p.bins, bin, bin != RCX_PICK_NONE);
    }
}

__global__ __launch_bounds__(RCX_PICK_SCAN_THREADS) void rcx_picks_scan_k(const RcxPickPlan p)
{
    __shared__ u32 lds[RCX_PICK_SCAN_THREADS / 64u];
    (void)rcx_bins_scan<RCX_PICK_BINS>(p.bins, lds, [&](u32 b, u32 before, u32 mine) {
        p.cursor[b] = before;
        if (b == RCX_PICK_CODED_BINS) {
            p.counts[0] = before;
            p.counts[1] = mine;
        }
        if (b == RCX_PICK_CODED_BINS + 1u) p.counts[2] = mine;
    });
}

__global__ __launch_bounds__(RCX_PICK_THREADS) void rcx_picks_scatter_k(const RcxPickTables t, const RcxPickPlan p)
{
    const u64 count = rcx_pick_count(t.count, t.max_pick);
    for (u64 k0 = (u64)blockIdx.x * RCX_PICK_THREADS; k0 < count; k0 += (u64)gridDim.x * RCX_PICK_THREADS) {
        const u64 k = k0 + threadIdx.x;
        const u32 bin = k < count ? p.keys[k] : RCX_PICK_NONE;
        const bool has = bin != RCX_PICK_NONE;
        const u32 w = rcx_pick_take(p.cursor, bin, has);
        if (has && (u64)w < t.max_pick) { // (the bins hold at most `count` entries between them)
            p.at[w] = t.dst_at[k];
            p.len[w] = (u32)t.dst_len[k];
            p.id[w] = (u32)k;
            p.stream[w] = (u32)t.pick[k];
        }
    }
}

// The stored picks as entries of rcx_stored_copy_k, which is launched for 2 * max_pick entries of which the first max_pick
// are long: entry e < max_pick is the e-th long stored pick if there are that many, entry max_pick + e the e-th short one.
// The planner has looked at the stream's length.
struct RcxCountedPickEntries {
    const u8* comp;
    const u64* comp_offsets;
    u8* dst;
    const u32* counts;
    u64 max_pick;
    RcxItems g;
    __device__ __forceinline__ bool find(u64 e, bool, const u8*& from, u8*& to, u32& len) const
    {
        const u64 ncoded = counts[0], nlong = counts[1], nshort = counts[2];
        u64 w;
        if (e < max_pick) {
            if (e >= nlong) return false;
            w = ncoded + e;
        } else {
            if (e - max_pick >= nshort) return false;
            w = ncoded + nlong + (e - max_pick);
        }
        if (w >= max_pick) return false;
        len = g.len[w];
        from = comp + comp_offsets[g.stream[w]];
        to = dst + g.at[w];
        return true;
    }
};

#endif // !RCX_HOST_SIM
