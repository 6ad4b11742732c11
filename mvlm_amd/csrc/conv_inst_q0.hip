// Instantiates the F(4,3) Winograd tile on its 32 x 16 workgroup shape (conv_variants.h: MVLM_CONV_WINO4_CFG; variant code
// MVLM_CONV_VARIANT_WINO4).  Which launches come here, which go to the wide shape (conv_inst_q1.hip) and which arrive with padded
// weights is the dispatcher's decision (conv_mfma.hip: f43_plan).
#include "conv_kernel.h"
#include "conv_variants.h"

int mvlm_conv_launch_wino4_narrow(mvlm_ctx* ctx, const ConvArgs& a) { return launch_variant<MVLM_CONV_WINO4_CFG>(ctx, a, MVLM_CONV_WINO4_ATTR_BIT); }
