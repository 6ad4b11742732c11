// Instantiates group 3 of the convolution kernel variants (conv_variants.h).
#include "conv_kernel.h"
#include "conv_variants.h"

// conv_inst_q0.hip: an eligible launch of the 80-row tile runs on the F(4,3) Winograd tile over weights padded to whole 32-channel columns
bool mvlm_conv_wino4_padded_takes(const mvlm_ctx* ctx, const ConvArgs& a);
int mvlm_conv_launch_wino4_padded(mvlm_ctx* ctx, const ConvArgs& a);

#define X(id, name, ...) \
    int mvlm_conv_launch_##id(mvlm_ctx* ctx, const ConvArgs& a) { return mvlm_conv_wino4_padded_takes(ctx, a) ? mvlm_conv_launch_wino4_padded(ctx, a) : launch_variant<__VA_ARGS__>(ctx, a, id); } \
    int mvlm_conv_pair_launch_##id(mvlm_ctx* ctx, const ConvArgs& a0, const ConvArgs& a1) { return launch_variant_pair<__VA_ARGS__>(ctx, a0, a1, id); }
MVLM_CONV_VARIANTS_G3(X)
#undef X
