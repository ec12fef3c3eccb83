// ltr_mlp.hip -- translation unit of the fused MLP scorer + loss kernels (ltr_mlp.inc, ltr_mlp2.inc, ltr_mlp_listwise.inc),
// the stand-alone MLP scorer (shared layer: ltr_mlp_stream.inc; f32 rows: ltr_mlp_rows.inc; bf16 features: ltr_mlp_bf16.inc;
// wide rows: ltr_mlp_wide.inc) and the stand-alone Linear scorer on f32 and bf16 rows (ltr_scorer.inc: one streaming layer
// under both element types, which shares the MLP's reduction kernel).
#include "ltr_common.inc"
// the listwise slot of the training step: the ranked row (layout, ranking, scans), the ListMLE and LambdaRank row functions
#define LTR_RANKED_ROW_ONLY
// In this translation unit the row helpers read the thread index through an empty asm (row_tid(), ltr_ranked.inc).  As
// plain threadIdx.x reads their lane-derived LDS addresses are loop invariants of the MLP kernels' query loop: hoisted
// in front of it they live across the MFMA chains, and the widest bucket of the tile kernel spills (ListMLE: up to 28
// VGPRs).  Opaque, that arithmetic is redone in the loss slot of every query (its cost per query has not
// been measured).  Same values, same results.
#define LTR_ROW_TID_OPAQUE
#include "ltr_ranked.inc"
#include "ltr_listmle_row.inc"
#include "ltr_lambdarank_row.inc"
#include "ltr_mlp.inc"
// the training step with the optimizer update in the reduction launch (include/ltr_mlp_train.h)
#include "ltr_mlp_train.inc"
#include "ltr_mlp_stream.inc"
#include "ltr_mlp_rows.inc"
#include "ltr_mlp_bf16.inc"
#include "ltr_mlp_wide.inc"
#include "ltr_scorer.inc"
