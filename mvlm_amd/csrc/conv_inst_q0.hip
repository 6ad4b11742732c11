// Instantiates the F(4,3) Winograd tile (conv_variants.h: MVLM_CONV_WINO4_CFG; variant code MVLM_CONV_VARIANT_WINO4).
#include "conv_kernel.h"
#include "conv_variants.h"
#include "conv_wino4_wide_hold.h"
#include "conv_tuned_wino4_pad.h"

int mvlm_conv_launch_wino4_wide(mvlm_ctx* ctx, const ConvArgs& a);  // the wide shape's, defined in conv_inst_q1.hip

// a (shape, kind) that ran slower on the wide shape inside the network (conv_wino4_wide_hold.h) stays on the 32 x 16 shape
static bool wide_shape_held(const ConvArgs& a) {
    const int kind = mvlm_conv_kind(a);
    for (int i = 0; i < MVLM_CONV_WINO4_WIDE_HOLD_N; ++i) {
        const ConvWino4WideHold& e = MVLM_CONV_WINO4_WIDE_HOLD[i];
        if (e.cin_pad == a.cin_pad && e.cout_pad == a.cout_pad && e.size == a.H && e.kind == kind) return true;
    }
    return false;
}

// Code 2048's launcher chooses the workgroup shape: the wide one where the context's switch is on and the output channels come in 64s
int mvlm_conv_launch_wino4(mvlm_ctx* ctx, const ConvArgs& a) {
    if (ctx->conv_winograd4_wide && mvlm_conv_wino4_wide_shape_ok(a.cout_pad, a.H) && !wide_shape_held(a)) return mvlm_conv_launch_wino4_wide(ctx, a);
    return launch_variant<MVLM_CONV_WINO4_CFG>(ctx, a, MVLM_CONV_WINO4_ATTR_BIT);
}

// ---- the 80- and 84-row direct tiles' launches on this tile (variants 16 and 26: conv_inst_g3.hip, conv_inst_g12.hip) -------------
// Such a layer's cout_pad is no multiple of 32, so the dispatcher never sends it here (tile_fits).  Its launcher does, below the
// dispatcher, where the launch carries weights and bias padded to whole 32-channel columns (ConvArgs::wino4_pad): the kernel guards
// every store by cout, and the columns beyond cout_pad multiply zeros.
bool mvlm_conv_wino4_padded_takes(const mvlm_ctx* ctx, const ConvArgs& a) {
    if (a.wino4_pad <= 0 || size_t(a.wino4_pad) > ctx->conv_wino4_pads.size() || !ctx->conv_wino4_pads[size_t(a.wino4_pad) - 1].w) return false;
    // a plain 3x3 layer writing a plain tensor, as the two direct tiles serve it
    if (a.ksize != 3 || a.up_in || a.in2 || a.amax_val || a.res1 || a.res2 || a.post_scale || a.out_raw || a.pool_out || a.up_out || !a.out || a.n_par != 1 ||
        a.kparts > 1 || a.H != a.W || a.H % 16 != 0 || a.cin_pad > 256 || (a.bias && !ctx->conv_wino4_pads[size_t(a.wino4_pad) - 1].bias))
        return false;
    if (ctx->conv_force_variant >= 0) return false;  // tools and tests force 16 / 26 to get the direct tile
    if (ctx->conv_winograd == 0 || ctx->conv_winograd4 == 0 || ctx->conv_winograd4_padded == 0) return false;
    if (ctx->conv_winograd4_padded == 2) return true;
    const int kind = mvlm_conv_kind(a);
    for (int i = 0; i < MVLM_CONV_TUNED_WINO4_PAD_N; ++i) {
        const ConvTunedWino4Pad& e = MVLM_CONV_TUNED_WINO4_PAD[i];
        if (e.cin_pad == a.cin_pad && e.cout_pad == a.cout_pad && e.size == a.H && e.kind == kind && a.B >= e.min_batch) return true;
    }
    return false;
}

int mvlm_conv_launch_wino4_padded(mvlm_ctx* ctx, const ConvArgs& a) {
    const ConvWino4Pad& p = ctx->conv_wino4_pads[size_t(a.wino4_pad) - 1];
    ConvArgs b = a;
    b.w = p.w;
    b.bias = a.bias ? p.bias : nullptr;
    b.cout_pad = mvlm_conv_wino4_padded_cout(a.cout_pad);  // (cout stays: the epilogue stores no channel beyond it)
    if (launch_variant<MVLM_CONV_WINO4_CFG>(ctx, b, MVLM_CONV_WINO4_ATTR_BIT)) return 1;
    ++ctx->conv_wino4_padded_launches;
    ctx->conv_launch_ran_as = MVLM_CONV_VARIANT_WINO4;
    return 0;
}
