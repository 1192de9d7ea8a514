// facade_test.cpp -- drives include/cpprcoder_amd/cpprcoder.h the way the reference harness drives
// cpprcoder.h (test/main.cpp:321-344) and the way its disabled unit test does (test/main.cpp:1200-1238).
// Built and run by tests/test_gpu_facade.py on the GPU box; results go to stdout / an output file and
// are compared with the oracle there.
//
//   facade_test enc  <in> <out> <sink_capacity> <piece>   piece: 0 = one call, N = pieces of N bytes, -1 = encode(u8)
//   facade_test enct <in> <out> <sink_capacity> <piece>   as enc in pieces of N bytes; prints the sink's size after initialize()
//                                                         and after every encode() call (what a caller sees between calls)
//   facade_test dec  <in> <out> <sink_capacity> <piece>
//   facade_test senc|sdec <in> <out> <sink_capacity>       static RangeEncoder<>::encode / decode
//   facade_test blocks <in> <out> <block>                  BlockCoder round trip; out = compacted streams
//   facade_test renc|rdec <in> <out> <size> <simd>         cppans::rANS::encode(_simd) / decode(_simd), test/main.cpp:384-387
//   facade_test benc|bdec <in> <out> 0                     blksort::BlkSort::encode / decode, test/main.cpp:812-825
//   facade_test threads <in> <out> <T> <block>             T threads, thread t on the t-th slice of the input: every facade
//                                                         twice over (thread 0 three times), see run_slice below
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cpprcoder_amd/blksort.h"
#include "cpprcoder_amd/cppans.h"
#include "cpprcoder_amd/cpprcoder.h"

static std::vector<cpprcoder::u8> slurp(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<cpprcoder::u8>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void dump(const char* path, const cpprcoder::u8* p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n));
}

// ---- mode `threads` ------------------------------------------------------------------------------------------------------
// What one thread does with its slice, `passes` times over (the second pass meets the thread's warm thread_local contexts;
// thread 0 does one pass more than the others, so that their contexts are destroyed -- the Holders' destructors run
// rcx_ctx_destroy as each thread ends -- while it is still coding):
//   1. BlockCoder(block).encode / decode of the slice
//   2. AdaptiveRangeEncoder<MemoryStream> / AdaptiveRangeDecoder<MemoryStream> on its first 20 000 bytes in pieces of 777
//   3. cppans::rANS::encode / decode and encode_simd / decode_simd on its first 30 000 bytes
//   4. blksort::BlkSort encode / decode on its first 3 * 32768 bytes
// The results of the last pass are the thread's region of <out>: the block payload, the offsets (8 bytes each, as they lie
// in memory), the adaptive stream, the two rANS streams, the sorted blocks.  Its line on stdout:
//   t passes failed  payload offsets  enc_status enc_request enc_size dec_status dec_request  rans_size rans_ret rans8_size rans8_ret  bwt_size bwt_ok
// `failed` counts the round trips that did not return the slice, and the results that differ from the pass before.
struct SliceResult {
    std::vector<cpprcoder::u8> region;
    int failed = 0;
};

static void append(std::vector<cpprcoder::u8>& to, const void* p, size_t n)
{
    const cpprcoder::u8* b = static_cast<const cpprcoder::u8*>(p);
    to.insert(to.end(), b, b + n);
}

static std::mutex g_print;

static void run_slice(int t, int passes, const cpprcoder::u8* slice, size_t size, cpprcoder::u32 block, SliceResult* result)
{
    using namespace cpprcoder;
    std::vector<u8> last;
    std::string last_line;
    int failed = 0;
    for (int pass = 0; pass < passes; ++pass) {
        std::vector<u8> region;
        char line[512];
        // 1. the block coder
        std::vector<u8> comp, back;
        std::vector<u64> offsets;
        {
            BlockCoder coder(block);
            if (!coder.encode(comp, offsets, size, slice) || !coder.decode(back, comp, offsets) || back.size() != size ||
                memcmp(back.data(), slice, size) != 0)
                ++failed;
        }
        append(region, comp.data(), comp.size());
        append(region, offsets.data(), offsets.size() * sizeof(u64));
        // 2. the adaptive coder, piece by piece
        const size_t an = size < 20000 ? size : 20000;
        Result er = {Status_Error, 0}, dr = {Status_Pending, 0};
        s32 enc_size = 0;
        {
            MemoryStream sink(static_cast<s32>(an + an / 32 + 1024));
            AdaptiveRangeEncoder<MemoryStream> enc;
            if (!enc.initialize(sink, static_cast<u32>(an))) ++failed;
            for (size_t at = 0; at < an; at += 777) er = enc.encode(static_cast<s32>(an - at < 777 ? an - at : 777), slice + at);
            enc_size = sink.size();
            append(region, sink.get(), static_cast<size_t>(sink.size()));
            MemoryStream plain(static_cast<s32>(an < 16 ? 16 : an));
            AdaptiveRangeDecoder<MemoryStream> dec;
            dec.initialize(plain);
            for (s32 at = 0; at < enc_size; at += 777) {
                dr = dec.decode(enc_size - at < 777 ? enc_size - at : 777, sink.get() + at);
                if (dr.status_ != Status_Pending) break;
            }
            if (static_cast<size_t>(plain.size()) != an || memcmp(plain.get(), slice, an) != 0) ++failed;
        }
        // 3. rANS, one state and eight
        const u32 rn = static_cast<u32>(size < 30000 ? size : 30000);
        u32 rsize[2] = {0, 0}, rret[2] = {0, 0};
        for (int simd = 0; simd < 2; ++simd) {
            const u32 cap = static_cast<u32>(cppans::rANS::calc_encoded_size(rn));
            std::vector<u8> dst(cap), plain(rn);
            rsize[simd] = simd ? cppans::rANS::encode_simd(cap, dst.data(), rn, slice) : cppans::rANS::encode(cap, dst.data(), rn, slice);
            const u8* stream = dst.data() + cap - rsize[simd]; // the stream is the END of the destination
            rret[simd] = simd ? cppans::rANS::decode_simd(rn, plain.data(), rsize[simd], stream) : cppans::rANS::decode(rn, plain.data(), rsize[simd], stream);
            if (rsize[simd] == 0 || memcmp(plain.data(), slice, rn) != 0) ++failed;
            append(region, stream, rsize[simd]);
        }
        // 4. the block sort
        const uint32_t bn = static_cast<uint32_t>(size < 3 * 32768 ? size : 3 * 32768);
        const uint32_t room = blksort::BlkSort::encodeBound(bn);
        int bwt_ok = 1;
        {
            std::vector<u8> sorted(room), plain(bn);
            blksort::BlkSort blk;
            blk.encode(bn, sorted.data(), slice);
            bwt_ok = bwt_ok && blk.ok();
            blk.decode(room, plain.data(), sorted.data());
            bwt_ok = bwt_ok && blk.ok();
            if (!bwt_ok || memcmp(plain.data(), slice, bn) != 0) ++failed;
            append(region, sorted.data(), sorted.size());
        }
        snprintf(line, sizeof(line), "%zu %zu  %d %u %d %d %u  %u %u %u %u  %u %d", comp.size(), offsets.size(), static_cast<int>(er.status_),
                 er.requestSize_, enc_size, static_cast<int>(dr.status_), dr.requestSize_, rsize[0], rret[0], rsize[1], rret[1], room, bwt_ok);
        if (pass && (region != last || last_line != line)) ++failed; // the warm context gives what the fresh one gave
        last.swap(region);
        last_line = line;
    }
    result->region.swap(last);
    result->failed = failed;
    std::lock_guard<std::mutex> g(g_print);
    printf("%d %d %d  %s\n", t, passes, failed, last_line.c_str());
}

static int run_threads(const std::vector<cpprcoder::u8>& in, const char* out_path, int T, cpprcoder::u32 block)
{
    if (T < 1 || T > 16) return 2;
    const size_t size = in.size() / static_cast<size_t>(T);
    std::vector<SliceResult> results(static_cast<size_t>(T));
    std::vector<std::thread> threads;
    for (int t = 0; t < T; ++t) threads.emplace_back(run_slice, t, t == 0 ? 3 : 2, in.data() + static_cast<size_t>(t) * size, size, block, &results[t]);
    for (auto& th : threads) th.join();
    std::vector<cpprcoder::u8> all;
    int failed = 0;
    for (auto& r : results) {
        all.insert(all.end(), r.region.begin(), r.region.end());
        failed += r.failed;
    }
    dump(out_path, all.data(), all.size());
    return failed ? 7 : 0;
}

int main(int argc, char** argv)
{
    using namespace cpprcoder;
    if (argc < 5) return 2;
    std::vector<u8> in = slurp(argv[2]);
    if (!strcmp(argv[1], "threads")) return argc < 6 ? 2 : run_threads(in, argv[3], atoi(argv[4]), static_cast<u32>(atoi(argv[5])));
    if (!strcmp(argv[1], "enc")) {
        s32 cap = atoi(argv[4]);
        int piece = atoi(argv[5]);
        MemoryStream sink(cap);
        AdaptiveRangeEncoder<> enc;
        if (!enc.initialize(sink, static_cast<u32>(in.size()))) return 3;
        Result r = {Status_Success, 0};
        if (piece == 0 || in.empty()) {
            r = enc.encode(static_cast<s32>(in.size()), in.data());
        } else if (piece < 0) {
            for (size_t i = 0; i < in.size(); ++i) r = enc.encode(in[i]);
        } else {
            for (size_t at = 0; at < in.size(); at += piece) {
                size_t len = in.size() - at < static_cast<size_t>(piece) ? in.size() - at : piece;
                r = enc.encode(static_cast<s32>(len), in.data() + at);
            }
        }
        dump(argv[3], sink.get(), static_cast<size_t>(sink.size()));
        printf("%d %u %d %d\n", static_cast<int>(r.status_), r.requestSize_, sink.size(), sink.capacity());
        return 0;
    }
    if (!strcmp(argv[1], "enct")) {
        s32 cap = atoi(argv[4]);
        int piece = atoi(argv[5]);
        MemoryStream sink(cap);
        AdaptiveRangeEncoder<> enc;
        if (!enc.initialize(sink, static_cast<u32>(in.size()))) return 3;
        Result r = {Status_Success, 0};
        std::vector<s32> sizes(1, sink.size());
        if (in.empty()) {
            r = enc.encode(0, in.data());
            sizes.push_back(sink.size());
        }
        for (size_t at = 0; at < in.size();) {
            size_t len = in.size() - at < static_cast<size_t>(piece) ? in.size() - at : piece;
            r = enc.encode(static_cast<s32>(len), in.data() + at);
            at += len;
            sizes.push_back(sink.size());
            if (r.status_ == Status_Error || (r.status_ == Status_Pending && at < in.size() && r.requestSize_ != in.size() - at)) break; // the sink filled
        }
        dump(argv[3], sink.get(), static_cast<size_t>(sink.size()));
        printf("%d %u %d %d\n", static_cast<int>(r.status_), r.requestSize_, sink.size(), sink.capacity());
        for (size_t i = 0; i < sizes.size(); ++i) printf("%d ", sizes[i]);
        printf("\n");
        return 0;
    }
    if (!strcmp(argv[1], "dec")) {
        s32 cap = atoi(argv[4]);
        int piece = atoi(argv[5]);
        MemoryStream sink(cap);
        AdaptiveRangeDecoder<> dec;
        dec.initialize(sink);
        Result r = {Status_Pending, 0};
        if (piece <= 0) {
            r = dec.decode(static_cast<s32>(in.size()), in.data());
        } else {
            size_t at = 0;
            bool first = true;
            while (at < in.size()) {
                size_t len = in.size() - at < static_cast<size_t>(piece) ? in.size() - at : piece;
                if (first && len < 8) len = in.size() - at < 8 ? in.size() - at : 8;
                first = false;
                r = dec.decode(static_cast<s32>(len), in.data() + at);
                at += len;
                if (r.status_ != Status_Pending) break;
            }
        }
        dump(argv[3], sink.get(), static_cast<size_t>(sink.size()));
        printf("%d %u %d %d\n", static_cast<int>(r.status_), r.requestSize_, sink.size(), sink.capacity());
        return 0;
    }
    if (!strcmp(argv[1], "senc") || !strcmp(argv[1], "sdec")) { // static coder: test/main.cpp:270-283
        s32 cap = atoi(argv[4]);
        MemoryStream sink(cap);
        RangeEncoder<> coder;
        bool ok = !strcmp(argv[1], "senc") ? coder.encode(sink, static_cast<u32>(in.size()), in.data())
                                           : coder.decode(sink, static_cast<u32>(in.size()), in.data());
        dump(argv[3], sink.get(), static_cast<size_t>(sink.size()));
        printf("%d 0 %d %d\n", ok ? 1 : 0, sink.size(), sink.capacity());
        return 0;
    }
    if (!strcmp(argv[1], "renc")) { // the stream is the last `size` bytes of the destination (test/main.cpp:384-386)
        const bool simd = atoi(argv[5]) != 0;
        const cppans::u64 cap = atoi(argv[4]) > 0 ? static_cast<cppans::u64>(atoi(argv[4])) : cppans::rANS::calc_encoded_size(static_cast<u32>(in.size()));
        std::vector<u8> dst(static_cast<size_t>(cap));
        const u32 size = simd ? cppans::rANS::encode_simd(static_cast<u32>(cap), dst.data(), static_cast<u32>(in.size()), in.data())
                              : cppans::rANS::encode(static_cast<u32>(cap), dst.data(), static_cast<u32>(in.size()), in.data());
        dump(argv[3], dst.data() + cap - size, size);
        printf("%u %llu\n", size, static_cast<unsigned long long>(cap));
        return 0;
    }
    if (!strcmp(argv[1], "rdec")) {
        const bool simd = atoi(argv[5]) != 0;
        std::vector<u8> dst(static_cast<size_t>(atoi(argv[4])));
        const u32 ret = simd ? cppans::rANS::decode_simd(static_cast<u32>(dst.size()), dst.data(), static_cast<u32>(in.size()), in.data())
                             : cppans::rANS::decode(static_cast<u32>(dst.size()), dst.data(), static_cast<u32>(in.size()), in.data());
        dump(argv[3], dst.data(), dst.size());
        printf("%u %zu\n", ret, dst.size());
        return 0;
    }
    if (!strcmp(argv[1], "benc") || !strcmp(argv[1], "bdec")) { // run_blksort: test/main.cpp:812-825
        const bool forward = !strcmp(argv[1], "benc");
        const uint32_t size = static_cast<uint32_t>(in.size());
        // decode writes blocks * 32768 + rest bytes, blocks = size / 32770 (blksort.h:451-462)
        const uint32_t room = forward ? blksort::BlkSort::encodeBound(size) : static_cast<uint32_t>(rcx_bwt_decoded_size(size));
        std::vector<u8> dst(room);
        blksort::BlkSort blk;
        if (forward) blk.encode(size, dst.data(), in.data());
        else blk.decode(size, dst.data(), in.data());
        dump(argv[3], dst.data(), dst.size());
        printf("%d %u %u\n", blk.ok() ? 1 : 0, room, blksort::BlkSort::decodeBound(size));
        return 0;
    }
    if (!strcmp(argv[1], "blocks")) {
        u32 block = static_cast<u32>(atoi(argv[4]));
        BlockCoder coder(block);
        std::vector<u8> comp, back;
        std::vector<u64> offsets;
        if (!coder.encode(comp, offsets, in.size(), in.data())) return 4;
        if (!coder.decode(back, comp, offsets)) return 5;
        if (back != in) return 6;
        dump(argv[3], comp.data(), comp.size());
        printf("%zu %zu\n", comp.size(), offsets.size());
        return 0;
    }
    return 2;
}
