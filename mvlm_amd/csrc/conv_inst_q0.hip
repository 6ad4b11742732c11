// Instantiates the F(4,3) Winograd tile (conv_variants.h: MVLM_CONV_WINO4_CFG; variant code MVLM_CONV_VARIANT_WINO4).
#include "conv_kernel.h"
#include "conv_variants.h"
#include "conv_wino4_wide_hold.h"

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
