// ltr_linear_bf16.hip -- translation unit of the fused Linear(F, 1) step on bf16 feature batches of libltr_hip.so
// (include/ltr_linear_bf16.h); compiled next to ltr_kernels.hip, ltr_linear.hip and ltr_mlp.hip (pytorchltr_amd/build.py),
// so the four build in parallel.  The code is in the .inc file below; the streaming score and
// weight-gradient kernels on bf16 rows are in ltr_mlp.hip (ltr_scorer.inc), next to the f32 ones and the reduction kernel.
#include "ltr_common.inc"       // the C ABI's codes, the loss kinds' pair passes, partial_pitch, the bf16 vector helpers
#include "ltr_linear_bf16.inc"  // the register-tile fused step, its plan and its entry point
