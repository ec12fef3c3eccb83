// ltr_linear_bf16.hip -- translation unit of the Linear(F, 1) scorer on bf16 feature batches of libltr_hip.so
// (include/ltr_linear_bf16.h); compiled next to ltr_kernels.hip, ltr_linear.hip and ltr_mlp.hip (pytorchltr_amd/build.py),
// so the four build in parallel.  The code is in the .inc files below.
#include "ltr_common.inc"       // the C ABI's codes, the loss kinds' pair passes, partial_pitch
#include "ltr_linear_bf16.inc"  // the streaming score / gradient kernels, the register-tile fused step, their entry points
