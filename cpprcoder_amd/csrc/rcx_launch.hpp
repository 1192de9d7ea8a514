// rcx_launch.hpp -- which kernels code a set of work entries, and in which launch shape: the launch tables behind the
// block calls (rcx_api.hip), the host-buffer pipeline's chunks (rcx_host.hpp) and the item calls (rcx_items.hpp).
#pragma once
#include "rcx_ctx.hpp"

namespace
{

// Multi-wave workgroups (waves spread over the SIMDs of one CU) or single-wave ones (more waves per CU).
bool wide_workgroups(const rcx_ctx* c, u64 nblocks)
{
    (void)nblocks;
    return c->wide_wg != 0; // default: multi-wave (RCX_WIDE_WG=0 selects single-wave workgroups)
}

// Lanes per block for the adaptive decoder.  A wave-instruction costs its SIMD 4 cycles whatever it
// serves, so fewer lanes per block means less machine-wide work: with its waves placed one per SIMD
// (multi-wave workgroups) the quad kernel beats the octet kernel at every block count measured on 1 GiB
// (4 KiB ... 256 KiB blocks, profiles/r01s_decode_variants.jsonl).  The octet and one-lane kernels stay
// selectable.
int decode_lanes(const rcx_ctx* c, u64 nblocks)
{
    (void)nblocks;
    return c->lanes_per_block ? c->lanes_per_block : 4;
}

// Launch shape.  A wave-instruction costs its SIMD the same whatever its lanes do, and a block is one serial
// chain, so with few blocks the work is spread thin rather than packed: the multi-wave encoders carry
// `lanes` blocks per workgroup such that every CU has a workgroup before any carries 64, the quad decoders
// `quads` blocks per wave such that every SIMD has a wave before any carries 16.
u32 pow2_at_least(u64 x)
{
    u32 p = 1;
    while (p < x) p <<= 1;
    return p;
}
u32 encode_lanes(const rcx_ctx* c, u64 nblocks)
{
    if (c->enc_lanes) return (u32)c->enc_lanes;
    const u32 want = pow2_at_least(grid_for(nblocks, c->cus));
    return want > RCX_LANES ? RCX_LANES : want;
}
u32 decode_quads(const rcx_ctx* c, u64 nblocks)
{
    if (c->dec_quads) return (u32)c->dec_quads;
    const u32 want = pow2_at_least(grid_for(nblocks, 4ull * c->cus));
    return want > RCX_QUAD_BLOCKS ? RCX_QUAD_BLOCKS : want;
}

// Which part of the context's per-block scratch a set of launches uses, and in which launch shape.
struct ScratchRange {
    u64 first = 0;       // blocks into slots / sizes / starts / models / redo
    bool packed = false; // full workgroups and waves whatever the block count (chunks that share the machine)
};
struct ScratchView {
    u8* slots;
    u32* sizes;
    u32* starts;
    u32* models;
    u32* redo;
};

// The coding launches of pass 1 for `nblocks` work entries of geometry G (rcx_geom.hpp) whose scratch is `v`, slots `slot` bytes
// apart: all the blocks of a range (RcxBlocks), or the entries of one length class of an item call (RcxItems).
template <class G>
int encode_launches(rcx_ctx* c, int coder, const void* d_src, u64 n, u32 block, u64 nblocks, ScratchView v, u64 slot, hipStream_t s, bool packed, G g)
{
    const u8* const src = static_cast<const u8*>(d_src);
    const int variant = (G::items && c->enc_variant != 0) ? 3 : c->enc_variant; // (the superseded kernels of the diagnostic build know blocks only)
    // Static coder: with fewer than 32768 blocks (two one-wave workgroups per CU) the three-wave kernel, which
    // spreads 64 blocks over three SIMDs, is faster (157 vs 112 GB/s at 16384 blocks); with more, the one-wave
    // kernel fills the machine by itself (202 vs 157 GB/s at 32768 blocks).
    const bool static3 = coder == RCX_CODER_STATIC && variant >= 2 && nblocks < 32768;
    // The one-wave kernels, 64 blocks a wave: every block (redo = nullptr), or as the pass behind a multi-wave kernel
    // the blocks that one marked in `redo`.
    auto adaptive_pass = [&](const u32* redo) {
        hipLaunchKernelGGL((rcx_enc_adaptive_k<false, false, G>), dim3(grid_for(nblocks, RCX_LANES)), dim3(64), 0, s, src, n, block, nblocks, v.slots,
                           slot, v.sizes, c->divtab(), c->status, 0u, static_cast<u32*>(nullptr), redo, g);
    };
    auto static_pass = [&](const u32* redo) {
        hipLaunchKernelGGL(rcx_enc_static_k<G>, dim3(grid_for(nblocks, RCX_LANES)), dim3(64), 0, s, src, n, block, nblocks, v.slots, slot, v.sizes,
                           c->status, redo, g);
    };
    Timed t(c, s, RCX_T_ENCODE);
    if (is_rans(coder)) { // cppans.h: a block is an octet of lanes, four 8-block waves per workgroup
        const u32 grid = grid_for(nblocks, 4 * RCX_RANS_BLOCKS);
        if (coder == RCX_CODER_RANS8)
            hipLaunchKernelGGL((rcx_enc_rans_k<true, G>), dim3(grid), dim3(256), 0, s, src, n, block, nblocks, v.slots, slot, v.sizes, v.starts,
                               c->status, g);
        else {
            // one state per block = one chain per block: the model by octets, then the coding loop one lane per
            // block, `lanes` blocks per wave so that every SIMD has a wave before any wave carries 64
            hipLaunchKernelGGL((rcx_rans_model_k<14, G>), dim3(grid), dim3(256), 0, s, src, n, block, nblocks, v.models, g);
            // The coding loop: two waves per 64 blocks (coder, writer), 2 KiB of table per block: one workgroup per CU.
            // RCX_RANS1_WAVES=1 (diagnostic): the one-wave kernel it replaced, 16 blocks per wave (RCX_RANS1_LANES),
            // four waves per workgroup.
            const char* one = getenv("RCX_RANS1_WAVES");
            if (!(one && atoi(one) == 1)) {
                if (allow_lds(c, &rcx_enc_rans1w_k<G>, RCX_R1W_LDS_BYTES) != RCX_OK) return RCX_E_HIP;
                hipLaunchKernelGGL(rcx_enc_rans1w_k<G>, dim3(grid_for(nblocks, 64)), dim3(128), RCX_R1W_LDS_BYTES, s, src, n, block, nblocks,
                                   static_cast<const u32*>(v.models), v.slots, slot, v.sizes, v.starts, c->status, g);
            } else {
                u32 lanes = 16;
                if (const char* v2 = getenv("RCX_RANS1_LANES")) { const int q = atoi(v2); if (q == 1 || q == 2 || q == 4 || q == 8 || q == 16) lanes = (u32)q; }
                u32 lds_bytes = lanes * RCX_RANS1_ENC_WAVES * 2048u;
                // RCX_RANS1_ALONE=1 (diagnostic): more LDS than two workgroups have room for, so that thin workgroups are not
                // stacked on one CU
                if (getenv("RCX_RANS1_ALONE") && lds_bytes < 84u * 1024u) lds_bytes = 84u * 1024u;
                u32 lanes_shift = 0;
                while ((1u << lanes_shift) < lanes) ++lanes_shift;
                if (allow_lds(c, &rcx_enc_rans1_k<G>, 128 * 1024) != RCX_OK) return RCX_E_HIP;
                hipLaunchKernelGGL(rcx_enc_rans1_k<G>, dim3(grid_for(nblocks, (u64)lanes * RCX_RANS1_ENC_WAVES)), dim3(64 * RCX_RANS1_ENC_WAVES), lds_bytes,
                                   s, src, n, block, nblocks, static_cast<const u32*>(v.models), v.slots, slot, v.sizes, v.starts, c->status, lanes_shift, g);
            }
        }
    } else if (static3) {
        const u32 lanes = packed ? RCX_LANES : encode_lanes(c, nblocks);
        hipLaunchKernelGGL(rcx_enc_static3_k<G>, dim3(grid_for(nblocks, lanes)), dim3(RCX_ST3_THREADS), 0, s, src, n, block, nblocks, v.slots, slot,
                           v.sizes, c->status, v.redo, lanes, g);
        static_pass(v.redo); // (the second passes are part of the encode time: on adversarial data they are not free)
    } else if (coder == RCX_CODER_STATIC) {
        static_pass(nullptr);
    } else if (variant == 3) {
        const u32 lanes = packed ? RCX_LANES : encode_lanes(c, nblocks);
        hipLaunchKernelGGL(rcx_enc_mc5_k<G>, dim3(grid_for(nblocks, lanes)), dim3(RCX_MC5_THREADS), 0, s, src, n, block, nblocks, v.slots, slot,
                           v.sizes, c->divq(), c->status, v.redo, lanes, g);
        // Blocks in which a carry ran through more output bytes than the five-wave kernel keeps in LDS were
        // marked, not finished: the one-wave kernel encodes them again.  Nothing is marked on ordinary data
        // and every wave of this launch returns at once.
        adaptive_pass(v.redo);
#if defined(RCX_WITH_VARIANTS)
    } else if (variant == 2) {
        hipLaunchKernelGGL(rcx_enc_mc_k, dim3(grid_for(nblocks, RCX_LANES)), dim3(RCX_MC_THREADS), 0, s, src, n, block, nblocks, v.slots, slot,
                           v.sizes, c->divtab(), c->status);
    } else if (variant == 1) {
        hipLaunchKernelGGL(rcx_enc_oct_k, dim3(grid_for(nblocks, RCX_OCT_BLOCKS)), dim3(64), 0, s, src, n, block, nblocks, v.slots, slot, v.sizes,
                           c->divtab(), c->status);
#endif
    } else {
        adaptive_pass(nullptr);
    }
    return RCX_OK;
}

// The encode launches for blocks whose scratch (slots, sizes, starts, models, redo) begins `rg.first` blocks into the
// context's arrays, which the caller has reserved.  The many-block call is the whole range; the host-buffer
// pipeline (rcx_host.hpp) runs several chunks of one buffer at once, each on its own stream and its own part of the
// scratch, `packed` = every workgroup / wave carries its full load of blocks, so that chunks share the machine.
int encode_range(rcx_ctx* c, int coder, const void* d_src, u64 n, u32 block, void* d_dst, u64 dst_cap, u64* d_offsets, hipStream_t s,
                 ScratchRange rg)
{
    const u64 nblocks = rcx_block_count(n, block);
    const u64 slot = rcx_block_bound_for(coder, block);
    ScratchView v{c->slots + rg.first * slot, c->sizes + rg.first, c->starts ? c->starts + rg.first : nullptr,
                  c->models ? c->models + rg.first * RCX_RANS_MODEL_DW : nullptr, c->redo + rg.first};
    {
        const int e = encode_launches(c, coder, d_src, n, block, nblocks, v, slot, s, rg.packed, RcxBlocks{});
        if (e != RCX_OK) return e;
    }
    {
        Timed t(c, s, RCX_T_SCAN);
        hipLaunchKernelGGL(rcx_scan_sizes_k, dim3(1), dim3(1024), 0, s, v.sizes, nblocks, d_offsets, dst_cap, c->status);
    }
    {
        Timed t(c, s, RCX_T_SCATTER);
        hipLaunchKernelGGL(rcx_scatter_k, dim3((u32)nblocks), dim3(256), 0, s, v.slots, slot, v.sizes, d_offsets,
                           static_cast<u8*>(d_dst), dst_cap, is_rans(coder) ? static_cast<const u32*>(v.starts) : static_cast<const u32*>(nullptr));
    }
    return LAUNCHED();
}

// The decode launches for `nblocks` work entries of geometry G (see encode_launches); `redo` = their marks.
template <class G>
int decode_launches(rcx_ctx* c, int coder, const void* d_comp, u64 comp_size, const u64* d_offsets, u64 nblocks, u32 block, u64 n, void* d_dst,
                    hipStream_t s, u32* redo, bool packed, G g)
{
    const u8* const comp = static_cast<const u8*>(d_comp);
    u8* const dst = static_cast<u8*>(d_dst);
    const int lanes_per = (G::items && decode_lanes(c, nblocks) == 8) ? 4 : decode_lanes(c, nblocks); // (the octet kernel of the diagnostic build knows blocks only)
    const u32 quads = packed ? RCX_QUAD_BLOCKS : decode_quads(c, nblocks); // blocks per wave of the 4-lane kernels
    const u32 quad_grid = grid_for(nblocks, (u64)quads * RCX_QUAD_DEC_WAVES), quad_threads = 64 * RCX_QUAD_DEC_WAVES;
    // The one-lane kernels, 64 blocks a wave: every block (marks = nullptr), or as the pass behind a 4-lane kernel the
    // blocks that one marked in `redo`.
    auto adaptive_pass = [&](const u32* marks) {
        hipLaunchKernelGGL((rcx_dec_adaptive_k<false, false, G>), dim3(grid_for(nblocks, RCX_LANES)), dim3(64), 0, s, comp, comp_size, d_offsets, nblocks,
                           block, n, dst, c->divtab(), c->status, static_cast<u32*>(nullptr), marks, g);
    };
    auto static_pass = [&](const u32* marks) {
        hipLaunchKernelGGL((rcx_dec_static_k<false, G>), dim3(grid_for(nblocks, RCX_LANES)), dim3(64), 0, s, comp, comp_size, d_offsets, nblocks, block, n,
                           dst, c->status, static_cast<u32*>(nullptr), marks, g);
    };
    Timed t(c, s, RCX_T_DECODE);
    if (coder == RCX_CODER_RANS8) {
        hipLaunchKernelGGL((rcx_dec_rans8_k<4, G>), dim3(grid_for(nblocks, 4 * RCX_RANS_BLOCKS)), dim3(256), 0, s, comp, comp_size, d_offsets, nblocks,
                           block, n, dst, c->status, g);
    } else if (coder == RCX_CODER_RANS) {
        hipLaunchKernelGGL((rcx_dec_rans1_quad_k<RCX_QUAD_DEC_WAVES, G>), dim3(quad_grid), dim3(quad_threads), 0, s, comp, comp_size, d_offsets, nblocks,
                           block, n, dst, c->status, quads, c->rans_track ? c->status + 2 : static_cast<u32*>(nullptr), g);
    } else if (coder == RCX_CODER_STATIC && lanes_per != 1) {
        hipLaunchKernelGGL((rcx_dec_static_quad_k<RCX_QUAD_DEC_WAVES, G>), dim3(quad_grid), dim3(quad_threads), 0, s, comp, comp_size, d_offsets, nblocks,
                           block, n, dst, c->status, redo, quads, g);
        static_pass(redo); // a target past the table or a symbol of count 0: see the adaptive coder's below
    } else if (coder == RCX_CODER_STATIC) {
        static_pass(nullptr);
    } else if (lanes_per == 4) {
        if (wide_workgroups(c, nblocks))
            hipLaunchKernelGGL((rcx_dec_quad_k<RCX_QUAD_DEC_WAVES, G>), dim3(quad_grid), dim3(quad_threads), 0, s, comp, comp_size, d_offsets, nblocks,
                               block, n, dst, c->divq(), c->status, redo, quads, g);
        else
            hipLaunchKernelGGL((rcx_dec_quad_k<1, G>), dim3(grid_for(nblocks, quads)), dim3(64), 0, s, comp, comp_size, d_offsets, nblocks, block, n, dst,
                               c->divq(), c->status, redo, quads, g);
        // Blocks whose stream asked for a symbol past the table (corrupt input) were marked, not decoded, by
        // the quad kernel: the one-lane kernel, which has the reference's fall-through for that case, decodes
        // them again.  On valid input nothing is marked and every wave of this launch returns at once.
        adaptive_pass(redo);
#if defined(RCX_WITH_VARIANTS)
    } else if (lanes_per == 8) {
        if (wide_workgroups(c, nblocks))
            hipLaunchKernelGGL(rcx_dec_oct_k<RCX_OCT_DEC_WAVES>, dim3(grid_for(nblocks, RCX_OCT_BLOCKS * RCX_OCT_DEC_WAVES)), dim3(64 * RCX_OCT_DEC_WAVES), 0, s,
                               comp, comp_size, d_offsets, nblocks, block, n, dst, c->divtab(), c->status);
        else
            hipLaunchKernelGGL(rcx_dec_oct_k<1>, dim3(grid_for(nblocks, RCX_OCT_BLOCKS)), dim3(64), 0, s, comp, comp_size, d_offsets, nblocks, block, n, dst,
                               c->divtab(), c->status);
#endif
    } else {
        adaptive_pass(nullptr);
    }
    return LAUNCHED();
}

// The decode launches for `nblocks` blocks whose redo marks begin `rg.first` entries into the context's array (see
// encode_range); the divisor table and the redo array are in place.
int decode_range(rcx_ctx* c, int coder, const void* d_comp, u64 comp_size, const u64* d_offsets, u64 nblocks, u32 block, u64 n, void* d_dst,
                 hipStream_t s, ScratchRange rg)
{
    u32* const redo = c->redo ? c->redo + rg.first : nullptr;
    return decode_launches(c, coder, d_comp, comp_size, d_offsets, nblocks, block, n, d_dst, s, redo, rg.packed, RcxBlocks{});
}

// The CRC-32 launch for `nblocks` work entries of geometry G (rcx_crc.hpp): d_expected == nullptr stores d_crc[id], else
// the entries are compared and a mismatch is latched.  One wave per entry, four to a workgroup; a workgroup copies 5 KiB
// of tables into LDS when it starts, so there are at most 8 per CU (32 waves, what a CU holds) and they loop over the entries.
template <class G>
int crc_launch(rcx_ctx* c, const void* d_src, u64 n, u32 block, u64 nblocks, u32* d_crc, const u32* d_expected, hipStream_t s, G g)
{
    const u8* const src = static_cast<const u8*>(d_src);
    const u64 want = (nblocks + RCX_CRC_WAVES - 1) / RCX_CRC_WAVES, most = 8ull * (u64)c->cus;
    const u32 grid = (u32)(want < most ? want : most);
    if (d_expected)
        hipLaunchKernelGGL((rcx_crc32_k<true, G>), dim3(grid), dim3(64 * RCX_CRC_WAVES), 0, s, src, n, block, nblocks, static_cast<u32*>(nullptr),
                           d_expected, c->status, g);
    else
        hipLaunchKernelGGL((rcx_crc32_k<false, G>), dim3(grid), dim3(64 * RCX_CRC_WAVES), 0, s, src, n, block, nblocks, d_crc,
                           static_cast<const u32*>(nullptr), c->status, g);
    return LAUNCHED();
}

} // namespace
