// rcx_ctx.hpp -- the context of include/rcx.h: its switches, its scratch and who sizes it, the timing scopes, and what
// every launch site uses (the grid of a launch, a kernel's leave for dynamic LDS).
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "rcx_buf.hpp"
#include "rcx_divtab.hpp"
#include "rcx_kernels.hpp"

struct EventPair {
    hipEvent_t a, b;
    int what;
};

struct HostPipe; // rcx_host.hpp: streams, threads' staging and bookkeeping of the host-buffer entry points

// What the host plans for an item call (rcx_items.hpp): the work order, its tables, the length classes of the scratch slots.
struct ItemClass {
    u64 first, count; // work entries
    u64 stride;       // bytes between their scratch slots
    u64 slot_base;    // where the class's slots begin in the context's slots
};

struct ItemPlan {
    std::vector<u64> at;
    std::vector<u32> len, id, stream, inv;
    std::vector<ItemClass> classes; // longest first (encode only)
    u64 nwork = 0, slots_bytes = 0;
    u32 longest = 0;
};

struct rcx_ctx {
    int device = 0;
    int lanes_per_block = 0; // decode: 0 = default (4, the quad kernel), 8 = octet, 4 = quad, 1 = one lane per block (RCX_LANES_PER_BLOCK)
    int wide_wg = -1;        // decode workgroups: -1/1 = multi-wave (default), 0 = single-wave (RCX_WIDE_WG)
    int enc_variant = 3;     // encode: 0 = one wave per 64 blocks, 1 = octet, 2 = 4-wave model/coder split, 3 = 5-wave split (RCX_ENC_VARIANT)
    int enc_lanes = 0;       // blocks per multi-wave encode workgroup: 0 = from the block count, else 1..64 (RCX_ENC_LANES)
    int dec_quads = 0;       // blocks per quad-decoder wave: 0 = from the block count, else 1, 2, 4, 8, 16 (RCX_DEC_QUADS)
    int cus = 256;           // compute units of the device
    std::vector<const void*> lds_allowed; // kernels that have been allowed their dynamic LDS (allow_lds)
    bool rans_track = false; // the single-stream rANS decode wants the payload bytes consumed (status[2])
    // scratch
    DevBuf<u8> slots;
    DevBuf<u32> sizes;
    DevBuf<u32> starts;      // rANS: where each block's stream begins in its slot (the encoders write backwards)
    DevBuf<u32> models;      // one-state rANS: every block's scaled cumulative counts + coding table (rcx_rans_model_k)
    DevBuf<u32> redo;        // decode: blocks the quad kernel leaves to the one-lane kernel (corrupt input only)
    DevBuf<u32> ties;        // block sort: [count, (block, period) ...] of the periodic blocks of the last forward call
    int bwt_atomic = -1;     // the block sort's counting passes rank with ds_add_rtn_u32 (1, checked on this device) or ballots (0); -1 = not asked yet
    // One allocation, two views: `div_entries` DivEntry, one per symbol of the largest block (divtab), and behind them the
    // same divisors as the quad decoder reads them, RCX_QUAD_DIVQ_DW words per group of 16 (divq; rcx_quad.hpp).
    DevBuf<u8> divmem;
    u64 div_entries = 0;
    u32 divtab_block = 0;
    DivEntry* divtab() const { return reinterpret_cast<DivEntry*>(divmem.get()); }
    u32* divq() const { return divmem ? reinterpret_cast<u32*>(divtab() + div_entries) : nullptr; }
    DevBuf<u8> itab;            // item calls: the work tables of the last call (rcx_items.hpp)
    std::vector<u64> itab_host; // ... as they are put together for the upload
    ItemPlan plan;              // ... and the plan they come from (kept for its vectors' capacity)
    DevBuf<u32> status;         // device: [flags, first bad block, track0, track1]
    PinBuf<u32> status_host;    // the same 4 words
    // staging for the host-pointer entry points
    DevBuf<u8> h_in, h_out;
    DevBuf<u64> h_off;
    HostPipe* pipe = nullptr;   // made by the first host-buffer call that is large enough to be cut into chunks
    // timing
    bool timing = false;
    std::vector<EventPair> pending;
    std::vector<EventPair> pool;
    double ms[RCX_T_COUNT] = {};
    uint64_t launches[RCX_T_COUNT] = {};
};

namespace
{

// Every entry point begins here.  Since HIP 7 an error code returned by ANY earlier runtime call of this thread -- the
// caller's, another library's -- stays in the thread's "last error" until somebody reads it, and the launches below are
// checked by reading it: what was there before is not ours to report (found by a test that ran after another one had left
// an error behind: the first kernel launch of the next call "failed").
inline hipError_t rcx_enter_device(int device)
{
    (void)hipGetLastError();
    return hipSetDevice(device);
}

struct Timed {
    rcx_ctx* c;
    hipStream_t s;
    EventPair p;
    bool on;
    Timed(rcx_ctx* ctx, hipStream_t st, int what) : c(ctx), s(st), on(ctx->timing)
    {
        if (!on) return;
        if (!c->pool.empty()) {
            p = c->pool.back();
            c->pool.pop_back();
        } else if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) {
            on = false;
            return;
        }
        p.what = what;
        (void)hipEventRecord(p.a, s);
    }
    ~Timed()
    {
        if (!on) return;
        (void)hipEventRecord(p.b, s);
        c->pending.push_back(p);
    }
};

// Workgroups for `entries` work entries, `per` to a workgroup.
inline u32 grid_for(u64 entries, u64 per) { return (u32)((entries + per - 1) / per); }

// More dynamic LDS than the 64 KiB a kernel gets without asking: asked for once per kernel and context.
template <class K>
int allow_lds(rcx_ctx* c, K* kernel, u32 bytes)
{
    const void* const f = reinterpret_cast<const void*>(kernel);
    if (std::find(c->lds_allowed.begin(), c->lds_allowed.end(), f) != c->lds_allowed.end()) return RCX_OK;
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    c->lds_allowed.push_back(f);
    return RCX_OK;
}

// Entry i serves total = 256 + i (rcx_divtab.hpp); built on the device, 16 bytes per symbol of the largest block, and
// 8 more for the quad decoder's copy: multiplier and increment (the addend is 0 or the multiplier), 16 entries a group.
__global__ void rcx_divtab_k(DivEntry* __restrict__ tab, u32* __restrict__ divq, u64 entries)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < entries) {
        const DivEntry e = rcx_make_div_entry((u32)(256 + i));
        tab[i] = e;
        u32* g = divq + (i >> 4) * RCX_QUAD_DIVQ_DW + (i & 15u);
        g[0] = e.mul;
        g[16] = e.add == 0 ? 0u : 1u;
    }
}

int ensure_divtab(rcx_ctx* c, u32 block)
{
    if (c->divmem && c->divtab_block >= block) return RCX_OK;
    // round up so that a sweep of block sizes builds the table once or twice
    u32 cover = 1u << 16;
    while (cover < block) cover <<= 1;
    const u64 entries = (u64)cover + 2 * RCX_STAGE; // a multiple of 16
    c->divmem.release();
    c->divtab_block = 0;
    c->div_entries = entries;
    if (c->divmem.reserve(entries * (sizeof(DivEntry) + 2 * sizeof(u32))) != RCX_OK) return RCX_E_NOMEM;
    hipLaunchKernelGGL(rcx_divtab_k, dim3(grid_for(entries, 256)), dim3(256), 0, nullptr, c->divtab(), c->divq(), entries);
    if (LAUNCHED() != RCX_OK || hipDeviceSynchronize() != hipSuccess) return RCX_E_HIP;
    c->divtab_block = cover;
    return RCX_OK;
}

bool block_ok(uint32_t block) { return block >= RCX_MIN_BLOCK && block <= RCX_MAX_BLOCK; }
bool is_rans(int coder) { return coder == RCX_CODER_RANS || coder == RCX_CODER_RANS8; }
bool coder_ok(int coder) { return coder == RCX_CODER_ADAPTIVE || coder == RCX_CODER_STATIC || is_rans(coder); }

int ensure_redo(rcx_ctx* c, u64 nblocks) { return c->redo.reserve(nblocks + 1); }

// The per-block scratch of `nwork` work entries whose slots take `slots_bytes` together (blocks: nwork slots of one size;
// items: rcx_items.hpp); the adaptive and static coders' divisor table covers blocks of `longest` symbols.
int reserve_scratch(rcx_ctx* c, int coder, u64 nwork, u64 slots_bytes, u32 longest)
{
    int r = is_rans(coder) ? RCX_OK : ensure_divtab(c, longest);
    if (r == RCX_OK) r = c->slots.reserve(slots_bytes + 256);
    if (r == RCX_OK) r = c->sizes.reserve(nwork + 1);
    if (r == RCX_OK && is_rans(coder)) r = c->starts.reserve(nwork + 1);
    if (r == RCX_OK && coder == RCX_CODER_RANS) r = c->models.reserve(nwork * RCX_RANS_MODEL_DW);
    return r == RCX_OK ? ensure_redo(c, nwork) : r;
}

int reserve(rcx_ctx* c, u64 n, u32 block, int coder = RCX_CODER_ADAPTIVE)
{
    const u64 nblocks = rcx_block_count(n, block);
    return reserve_scratch(c, coder, nblocks, nblocks * rcx_block_bound_for(coder, block), block);
}

// The staging of a host-buffer call: room for `in` and `out` bytes and `offs` table entries on the device.
int reserve_staging(rcx_ctx* c, u64 in, u64 out, u64 offs)
{
    int r = c->h_in.reserve(in + 64);
    if (r == RCX_OK) r = c->h_out.reserve(out + 64);
    return r == RCX_OK ? c->h_off.reserve(offs) : r;
}

} // namespace
