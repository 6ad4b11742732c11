// Instantiates the wide workgroup shape of the F(4,3) Winograd tile (conv_variants.h: MVLM_CONV_WINO4_WIDE_CFG), which
// the dispatcher (conv_mfma.hip: f43_plan) takes for launches of code MVLM_CONV_VARIANT_WINO4 with output channels in 64s.
#include "conv_kernel.h"
#include "conv_variants.h"

using WideCfg = MVLM_CONV_WINO4_WIDE_CFG;
static_assert(WideCfg::WIDE4 && WideCfg::PH == 12 && WideCfg::PLANE == 408 && WideCfg::XT == 1632 && WideCfg::WT == 4608 && WideCfg::STAGE == 6240);
static_assert(WideCfg::LDS_BYTES == 51968 && WideCfg::WJOBS == 272 && WideCfg::X_ITERS == 2 && WideCfg::W_ITERS == 5);
static_assert(WideCfg::MIN_BLOCKS_PER_CU == 2 && 2 * WideCfg::LDS_BYTES <= 160 * 1024, "two workgroups stay resident per CU");
static_assert(WideCfg::EMT == 1 && WideCfg::ENT == 4 && WideCfg::EPIX == 128 && WideCfg::ECOUT == 32, "a wave finishes one row quad of 32 channels");

int mvlm_conv_launch_wino4_wide(mvlm_ctx* ctx, const ConvArgs& a) { return launch_variant<WideCfg>(ctx, a, MVLM_CONV_WINO4_WIDE_ATTR_BIT); }
