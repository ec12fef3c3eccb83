// ltr_mlp.hip -- translation unit of the MLP scorer of libltr_hip.so (the fused training step, the stand-alone scorer) and of
// the stand-alone Linear scorer; compiled next to ltr_kernels.hip, ltr_linear.hip and ltr_linear_bf16.hip
// (pytorchltr_amd/build.py), so the four build in parallel.  This file is the table of contents: the code is in the .inc
// files below, each of which needs only what stands above it.
#include "ltr_common.inc"         // the C ABI's codes, the loss kinds' pair passes and LDS carve, block_sum, with_kind
// the listwise slot of the training step: the ranked row (layout, ranking, scans), the ListMLE and LambdaRank row functions
#define LTR_RANKED_ROW_ONLY
// In this translation unit the row helpers read the thread index through an empty asm (row_tid(), ltr_ranked.inc).  As
// plain threadIdx.x reads their lane-derived LDS addresses are loop invariants of the MLP kernels' query loop: hoisted
// in front of it they live across the MFMA chains, and the widest bucket of the tile kernel spills (ListMLE: up to 28
// VGPRs).  Opaque, that arithmetic is redone in the loss slot of every query (its cost per query has not
// been measured).  Same values, same results.
#define LTR_ROW_TID_OPAQUE
#include "ltr_ranked.inc"         // the ranked row; needs ltr_common.inc
#include "ltr_listmle_row.inc"    // the ListMLE row function; needs the ranked row
#include "ltr_lambdarank_row.inc" // the LambdaRank row function; needs the ranked row
#include "ltr_mlp_listwise.inc"   // MlpListwiseArgs and the ListNet / ListMLE / LambdaRank loss slots of both step kernels; needs the row functions
#include "ltr_mlp_reduce.inc"     // mlp_pitch, the two reduction cores over an epilogue, mlp_reduce_kernel / mlp_reduce4_kernel, mlp_reduce_launch; needs ltr_common.inc
#include "ltr_mlp.inc"            // MlpParams, the LDS sizes, mlp_schedule, the 8-wave kernel mlp_pairwise_kernel and its launchers; needs the loss slots
#include "ltr_mlp2.inc"           // the 4-wave tile kernel mlp_tile_kernel and its launchers; needs MlpParams, mlp_schedule and the loss slots
#include "ltr_mlp_step.inc"       // host: the layout choice, the slot dispatch, the launch path, the step's entry points; needs both kernels' launchers and mlp_reduce_launch
#include "ltr_mlp_train.inc"      // the optimizer update as the reduction's epilogue (include/ltr_mlp_train.h) and its entry points; needs the cores and the launch path
#include "ltr_mlp_stream.inc"     // the stand-alone MLP scorer's streaming core and host glue; needs MlpParams' helpers and mlp_reduce_launch
#include "ltr_mlp_rows.inc"       // f32 rows of any length; needs the streaming core
#include "ltr_mlp_bf16.inc"       // bf16 feature batches; needs the streaming core
#include "ltr_mlp_wide.inc"       // wide rows (K-streamed); needs the streaming core's host glue and mlp_reduce_launch
#include "ltr_scorer.inc"         // the stand-alone Linear scorer on f32 and bf16 rows; needs mlp_reduce_kernel
