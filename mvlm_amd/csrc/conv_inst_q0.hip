// Instantiates the F(4,3) Winograd tile (conv_variants.h: MVLM_CONV_WINO4_CFG; variant code MVLM_CONV_VARIANT_WINO4).
#include "conv_kernel.h"
#include "conv_variants.h"

int mvlm_conv_launch_wino4(mvlm_ctx* ctx, const ConvArgs& a) { return launch_variant<MVLM_CONV_WINO4_CFG>(ctx, a, MVLM_CONV_WINO4_ATTR_BIT); }
