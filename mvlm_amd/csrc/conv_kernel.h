// Kernel template of the implicit-GEMM convolution (see conv_mfma.hip for the overview); included by
// the translation units that instantiate groups of variants (conv_inst_g*.hip).  In reading order:
//   conv_cfg.h     Cfg<>: the tile geometry, constexpr arithmetic only (all the dispatcher takes)
//   conv_loop.h    the direct tiles' K loop: staging items and compute_chunk
//   conv_wino.h    the F(2,3) Winograd loop: WinoStage, compute_chunk_wino, wino_main
//   conv_wino4.h   the F(4,3) Winograd loop with its gap plan: Wino4Stage, Wino4Plan, gap_wino4, wino4_main
//   conv_tile.h    the workgroup program conv_tile and its two kernels
//   conv_launch.h  the host-side checks and launchers
#ifndef MVLM_CONV_KERNEL_H
#define MVLM_CONV_KERNEL_H
#include "conv_cfg.h"
#include "conv_loop.h"
#include "conv_wino.h"
#include "conv_wino4.h"
#include "conv_tile.h"
#include "conv_launch.h"
#endif
