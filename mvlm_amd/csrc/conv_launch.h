// Host side of a variant's kernels (conv_kernel.h lists the headers of the convolution kernel): the checks of one problem
// against the tile geometry, the dynamic-LDS attribute and the launches.
#ifndef MVLM_CONV_LAUNCH_H
#define MVLM_CONV_LAUNCH_H
#include <cstdlib>

#include "common.h"
#include "conv_tile.h"

namespace {

// ---- launchers -------------------------------------------------------------------------
struct ConvGrid {
    int tiles_x = 0, tiles_y = 0, cout_tiles = 0;
    long tiles = 0;  // output tiles (x parities); the grid has tiles * kparts workgroups
    long nblk = 0;
};

// host-side checks of one problem against a variant's tile geometry; fills the grid
template <class C>
int check_variant(mvlm_ctx* ctx, ConvArgs& a, ConvGrid& g) {
    const int tiles_x = a.W / C::TW, tiles_y = a.H / C::TRI;
    const int tiles_b = (a.B + C::NIMG - 1) / C::NIMG;
    const int cout_tiles = a.cout_pad / C::COUT_T;
    MVLM_REQUIRE(ctx, a.ksize == C::KS, "conv: kernel variant built for another kernel size");
    MVLM_REQUIRE(ctx, !a.in2 || (C::HAS_IN2 && !a.up_in && !a.amax_val && a.in_coff == 0 && a.in2_ctot >= a.cin && !(a.H & 1) && !(a.W & 1) && a.kparts <= 1),
                 "conv: a second input tensor (upsample + skip on the load) is served by the 128-channel 8x32 tile only");
    MVLM_REQUIRE(ctx, !C::WINO || (!a.up_in && !a.in2 && !a.amax_val && a.up_out != 2 && a.n_par == 1 && a.kparts <= 1),
                 "conv: the Winograd tiles serve plain, pooling and scattering 3x3 layers (no upsampled / second input, no fused argmax, no K parts)");
    MVLM_REQUIRE(ctx, !C::WINO4 || (!a.up_in && !a.in2 && !a.amax_val && a.up_out != 2 && a.n_par == 1 && a.kparts <= 1),
                 "conv: the F(4,3) Winograd tile serves plain, pooling and scattering 3x3 layers (no upsampled / second input, no fused argmax, no K parts)");
    MVLM_REQUIRE(ctx, a.W % C::TW == 0 && a.H % C::TRI == 0, "conv: spatial size not a multiple of the tile");
    MVLM_REQUIRE(ctx, !C::SPLITK || a.cin_pad % 32 == 0, "conv: split-K tiles need 32-channel chunks");
    MVLM_REQUIRE(ctx, !(C::SPLITK && C::NT > 1) || (a.kparts <= 1 && !a.amax_val), "conv: the two-column split-K tiles have no K-parts / argmax form");
    MVLM_REQUIRE(ctx, a.cout_pad % C::COUT_T == 0, "conv: cout_pad not a multiple of the cout tile");
    MVLM_REQUIRE(ctx, a.cin_pad % C::CK == 0, "conv: cin_pad must be a multiple of the K-chunk");
    MVLM_REQUIRE(ctx, !a.pre_scale || a.cin_pad <= C::BN_MAXC, "conv: pre-activation BatchNorm supports up to 256 input channels");
    MVLM_REQUIRE(ctx, !C::WINO || a.cin_pad <= C::BN_MAXC, "conv: the Winograd tiles keep a BatchNorm pair of every input channel in LDS, with or without pre-activation (up to 256)");
    MVLM_REQUIRE(ctx, !C::WINO4 || a.cin_pad <= C::BN_MAXC, "conv: the F(4,3) Winograd tile keeps a BatchNorm pair of every input channel in LDS, with or without pre-activation (up to 256)");
    if (C::TAIL4) MVLM_REQUIRE(ctx, a.up_out != 1 && (a.out || (a.amax_val && C::HAS_AMAX)), "conv: the 84-channel tile writes a plain (or parity) output tensor or argmax partials");
    if (C::TAIL16)
        MVLM_REQUIRE(ctx, !a.res1 && !a.res2 && !a.out_raw && !a.post_scale && a.up_out != 1 && !a.pool_out,
                     "conv: the 80-channel tiles serve plain conv + bias layers only");
    if (a.amax_val) {
        MVLM_REQUIRE(ctx, C::NIMG == 1, "conv: fused argmax needs one image per tile");
        MVLM_REQUIRE(ctx, a.amax_part0 >= 0 && a.amax_part0 + tiles_x * tiles_y * 4 <= a.amax_parts,
                     "conv: argmax partial range mismatch");
        MVLM_REQUIRE(ctx, !a.res1 && !a.post_scale && a.up_out != 1, "conv: fused argmax expects a plain conv + bias layer");
        MVLM_REQUIRE(ctx, !a.out && !a.out_raw && !a.pool_out, "conv: a fused-argmax launch does not materialise the heatmap");
    }
    long nblk = long(tiles_x) * tiles_y * tiles_b * cout_tiles;
    if (a.n_par != 1) {
        MVLM_REQUIRE(ctx, a.n_par == 4 && C::KS == 2 && a.up_out == 2, "conv: four parities per launch are a 2x2-kernel feature");
        MVLM_REQUIRE(ctx, a.w_par[0] && a.w_par[1] && a.w_par[2] && a.w_par[3], "conv: parity weights missing");
        MVLM_REQUIRE(ctx, !a.amax_val || (a.amax_par_stride >= tiles_x * tiles_y * 4 &&
                                          a.amax_part0 + 3 * a.amax_par_stride + tiles_x * tiles_y * 4 <= a.amax_parts),
                     "conv: argmax partial range mismatch (four parities)");
        nblk *= 4;
    }
    MVLM_REQUIRE(ctx, nblk > 0 && nblk < (1l << 31), "conv: bad grid");
    a.kparts = a.kparts > 1 ? a.kparts : 1;
    g.tiles = nblk;
    if (a.kparts > 1) {
        MVLM_REQUIRE(ctx, C::SPLITK, "conv: only the split-K tiles divide the input channels over workgroups");
        MVLM_REQUIRE(ctx, a.cin_pad % (a.kparts * C::CK) == 0, "conv: input channels do not divide into the requested K parts");
        nblk *= a.kparts;
    }
    MVLM_REQUIRE(ctx, nblk < (1l << 31), "conv: bad grid");
    g.tiles_x = tiles_x;
    g.tiles_y = tiles_y;
    g.cout_tiles = cout_tiles;
    g.nblk = nblk;
    return 0;
}

// dynamic-LDS limit of this variant's kernels: set once per context, i.e. per device (hipFuncSetAttribute
// applies to the current device's copy of the function; the ctx mutex held by every entry point guards the mask)
// attr_bit: the variant's bit of mvlm_ctx::conv_attr_mask (a base id, MVLM_CONV_WINO4_ATTR_BIT)
template <class C>
int set_variant_attributes(mvlm_ctx* ctx, int attr_bit) {
    if ((ctx->conv_attr_mask >> attr_bit) & 1ull) return 0;
    MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::HAS_AMAX)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::PAIRABLE)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_pair_kernel<C>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    if constexpr (C::HAS_IN2)
        MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false, true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(C::LDS_BYTES)));
    ctx->conv_attr_mask |= 1ull << attr_bit;
    return 0;
}

template <class C>
int launch_variant(mvlm_ctx* ctx, const ConvArgs& a_in, int attr_bit) {
    ConvArgs a = a_in;
#if defined(MVLM_CONV_TIMING)  // diagnostic build: the tool passes its counter buffer through the environment
    if (const char* e = getenv("MVLM_CONV_TIMING_BUF")) a.timing = reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    ConvGrid g;
    if (check_variant<C>(ctx, a, g)) return 1;
    if (a.kparts > 1) {
        MVLM_REQUIRE(ctx, g.tiles <= MVLM_KPARTS_MAX_TILES && g.nblk <= MVLM_KPARTS_MAX_PARTS, "conv: too many tiles for the K-part workspace");
        if (mvlm_conv_kparts_workspace(ctx, &a.kws, &a.kcnt)) return 1;
    }
    if (set_variant_attributes<C>(ctx, attr_bit)) return 1;
#if defined(MVLM_CONV_TIMING)  // diagnostic build: MVLM_CONV_TIMING_WINO4_LDS = dynamic LDS bytes an F(4,3) launch asks for at least.
    // More than half of a CU's 160 KiB leaves one workgroup per CU: the K loop's rate without a partner on the matrix pipe.
    if constexpr (C::WINO4) {
        if (const char* e = getenv("MVLM_CONV_TIMING_WINO4_LDS")) {
            const size_t lds = strtoull(e, nullptr, 0);
            if (lds > size_t(C::LDS_BYTES) && !a.amax_val && !a.in2) {
                MVLM_REQUIRE(ctx, lds <= 160 * 1024, "conv: MVLM_CONV_TIMING_WINO4_LDS beyond a CU's LDS");
                MVLM_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(conv_mfma_kernel<C, false>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
                hipLaunchKernelGGL((conv_mfma_kernel<C, false>), dim3((unsigned)g.nblk), dim3(256), lds, ctx->cur_stream(), a,
                                   g.tiles_x, g.tiles_y, g.cout_tiles);
                MVLM_CHECK_HIP(ctx, hipGetLastError());
                return 0;
            }
        }
    }
#endif
    if (a.amax_val) {
        if constexpr (C::HAS_AMAX) {
            hipLaunchKernelGGL((conv_mfma_kernel<C, true>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(),
                               a, g.tiles_x, g.tiles_y, g.cout_tiles);
        } else {
            return ctx->fail("conv: fused argmax is only built for the 8x32-pixel tile variants");
        }
    } else if (a.in2) {
        if constexpr (C::HAS_IN2) {
            hipLaunchKernelGGL((conv_mfma_kernel<C, false, true>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(), a,
                               g.tiles_x, g.tiles_y, g.cout_tiles);
        } else {
            return ctx->fail("conv: this kernel variant has no second-input form");
        }
    } else {
        hipLaunchKernelGGL((conv_mfma_kernel<C, false>), dim3((unsigned)g.nblk), dim3(256), C::LDS_BYTES, ctx->cur_stream(), a,
                           g.tiles_x, g.tiles_y, g.cout_tiles);
    }
    MVLM_CHECK_HIP(ctx, hipGetLastError());
    return 0;
}

// two independent convolutions on this variant's tiles in one grid (conv_pair_kernel); kparts of each problem in its ConvArgs
template <class C>
int launch_variant_pair(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1, int attr_bit) {
    if constexpr (!C::PAIRABLE) {
        return ctx->fail("conv: this kernel variant has no two-problem form");
    } else {
        ConvPairArgs p;
        p.a[0] = a0;
        p.a[1] = a1;
        ConvGrid g[2];
        for (int i = 0; i < 2; ++i) {
            ConvArgs& a = p.a[i];
            MVLM_REQUIRE(ctx, !a.amax_val && a.n_par == 1 && !a.timing && !a.in2, "conv: a paired launch takes plain convolutions");
            if (check_variant<C>(ctx, a, g[i])) return 1;
        }
        if (p.a[0].kparts > 1 || p.a[1].kparts > 1) {
            // one workspace per launch stream: problem 1's partial tiles and counters follow problem 0's
            const long t0 = p.a[0].kparts > 1 ? g[0].tiles : 0, n0 = p.a[0].kparts > 1 ? g[0].nblk : 0;
            const long t1 = p.a[1].kparts > 1 ? g[1].tiles : 0, n1 = p.a[1].kparts > 1 ? g[1].nblk : 0;
            MVLM_REQUIRE(ctx, t0 + t1 <= MVLM_KPARTS_MAX_TILES && n0 + n1 <= MVLM_KPARTS_MAX_PARTS, "conv: too many tiles for the K-part workspace");
            float* kws = nullptr;
            unsigned* kcnt = nullptr;
            if (mvlm_conv_kparts_workspace(ctx, &kws, &kcnt)) return 1;
            p.a[0].kws = kws;
            p.a[0].kcnt = kcnt;
            p.a[1].kws = kws + size_t(n0) * 1024;
            p.a[1].kcnt = kcnt + t0;
        }
        for (int i = 0; i < 2; ++i) {
            p.tiles_x[i] = g[i].tiles_x;
            p.tiles_y[i] = g[i].tiles_y;
            p.cout_tiles[i] = g[i].cout_tiles;
            p.nblk[i] = int(g[i].nblk);
        }
        p.nblk0_pad = (p.nblk[0] + 7) / 8 * 8;
        const long total = long(p.nblk0_pad) + p.nblk[1];
        MVLM_REQUIRE(ctx, total < (1l << 31), "conv: bad grid");
        if (set_variant_attributes<C>(ctx, attr_bit)) return 1;
        hipLaunchKernelGGL((conv_pair_kernel<C>), dim3((unsigned)total), dim3(256), C::LDS_BYTES, ctx->cur_stream(), p);
        MVLM_CHECK_HIP(ctx, hipGetLastError());
        return 0;
    }
}

}  // namespace
#endif
