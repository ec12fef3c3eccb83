/*
 * ltr_mlp_train.h -- C ABI of the fused MLP training step with the optimizer update inside the reduction launch.
 *
 * Exported by the same libltr_hip.so as include/ltr_hip.h, with its conventions: device pointers owned by the
 * caller, work enqueued on `stream` without host synchronisation, 0 = OK, < 0 = LTR_ERR_* (ltr_hip.h),
 * > 0 = a hipError_t; labels int64 / int32 / fp32 by `rel_dtype`, n int64 clamped to [0, L].
 */
#ifndef LTR_MLP_TRAIN_H
#define LTR_MLP_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the update rule */
#define LTR_OPT_SGD 0
#define LTR_OPT_ADAGRAD 1
#define LTR_OPT_ADAM 2

/* the loss family of a step: which of the three fused MLP entry points it repeats */
#define LTR_MLP_TRAIN_PAIRWISE 0   /* ltr_mlp_pairwise_f32 (ltr_hip.h):              code = kind, sigma              */
#define LTR_MLP_TRAIN_LISTWISE 1   /* ltr_mlp_listwise_f32 (ltr_listwise.h):         code = loss, k, the tie seed    */
#define LTR_MLP_TRAIN_LAMBDARANK 2 /* ltr_mlp_lambdarank_f32 (ltr_mlp_lambdarank.h): code ignored, k, sigma          */

/*
 * The hyper-parameters, torch.optim's names.  Doubles, as torch holds them: what a rule uses as an fp32 scalar is
 * rounded from the double once (the table below), what depends on the step count is evaluated in fp64.
 *   all:     algo, lr, weight_decay
 *   SGD:     momentum, dampening, nesterov
 *   Adagrad: lr_decay, eps
 *   Adam:    beta1, beta2, eps
 */
struct ltr_mlp_optim {
    int algo;
    int nesterov;
    double lr;
    double weight_decay;
    double momentum;
    double dampening;
    double lr_decay;
    double eps;
    double beta1;
    double beta2;
};

/*
 * The optimizer state: `nbuf` buffers of P = ltr_mlp_param_count(F, H1, H2) floats each, laid out like `grads`
 * ([W1 | b1 | W2 | b2 | W3 | b3], W1 rows of F floats), back to back, then the device header:
 *
 *     SGD      nbuf = 1: the momentum buffer (kept also for momentum 0, where it is never touched: one size per algo)
 *     Adagrad  nbuf = 1: `sum`
 *     Adam     nbuf = 2: `exp_avg`, then `exp_avg_sq`
 *
 *     header, at float offset LTR_MLP_TRAIN_HEADER_AT(nbuf * P) = nbuf * P rounded up to a multiple of 4 (so the header
 *     is 16-byte aligned where the state is), four 32-bit words:
 *         word 0  t, the number of steps taken (unsigned)
 *         word 1  the ticket word of the launch in flight; 0 between launches
 *         word 2, 3  reserved, 0
 *
 * ltr_mlp_train_state_floats returns LTR_MLP_TRAIN_HEADER_AT(nbuf * P) + 4, or 0 for an unknown algo or a bad network
 * (F, H1 or H2 <= 0).  The caller zeroes the whole state once (Adagrad with an initial accumulator value: fills `sum`
 * with it) and may read or write t between steps, in stream order (a restored checkpoint).
 */
#define LTR_MLP_TRAIN_HEADER_AT(floats) (((floats) + 3) & ~(size_t)3)
size_t ltr_mlp_train_state_floats(int algo, int F, int H1, int H2);

/*
 * One training step: the MFMA launch of the family's entry point, with the same arguments, then ONE reduce-and-update
 * launch in place of its reduction: the sum over the workgroups' partial vectors in the order of that reduction (the
 * gradient is bit for bit the one the entry point writes to `grads`), and, in the thread that holds a parameter's
 * gradient, the update of that parameter and of its state.
 *
 *   W1 .. b3: the six parameters, UPDATED IN PLACE.  `w1_pitch` is the row pitch of W1 in floats: F, or less where the
 *     batch was zero-padded to a multiple of 4 features -- then `W1_rows` is the zero-padded (H1, F) image of W1 that
 *     the MFMA launch reads, W1 itself receives the update, and the gradient columns >= w1_pitch (of the padding) are
 *     dropped.  W1_rows == NULL: W1 (needs w1_pitch == F).
 *   state: ltr_mlp_train_state_floats floats; may be NULL for SGD with momentum 0 (then no step is counted).
 *   grads_out (may be NULL): the summed gradient, ltr_mlp_param_count floats, as the entry point's `grads`.
 *   loss, scores_out, loss_sum, grad_out, workspace: as in the family's entry point.
 *
 * The rules are torch.optim's, in fp32, one parameter p with gradient g (t = word 0 before the step):
 *   SGD      g += wd * p;  with momentum mu: buf = g if t == 0 else mu * buf + (1 - dampening) * g;
 *            g = g + mu * buf if nesterov else buf;  p -= lr * g
 *   Adagrad  g += wd * p;  clr = lr / (1 + t * lr_decay);  sum += g * g;  p -= clr * (g / (sqrt(sum) + eps))
 *   Adam     g += wd * p;  m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * (g * g);
 *            p -= (lr / (1 - beta1^(t+1))) * (m / (sqrt(v) / sqrt(1 - beta2^(t+1)) + eps))
 *   The chain of fp32 roundings (what tests/mlp_train_ref.py counts): every product, sum, quotient and square root
 *   above is one fp32 operation (a product feeding a sum may be fused into one); wd, lr, mu, 1 - dampening, eps,
 *   beta1, 1 - beta1, beta2, 1 - beta2 are rounded to fp32 from the double; clr, lr / (1 - beta1^(t+1)) and
 *   sqrt(1 - beta2^(t+1)) are evaluated in fp64 once per workgroup and rounded to fp32.  Division and square root are
 *   the correctly rounded ones.  A term with a zero coefficient (wd, momentum) is left out, not added as 0.
 *   The last workgroup of the launch to take a ticket (an atomic add on word 1) stores t + 1 and resets the ticket;
 *   every workgroup reads t before it takes its ticket.  Nothing is allocated and the host reads nothing: a captured
 *   step replays correctly.  No atomics on floats: bit-identical run to run.
 *
 * Shapes, limits and errors are those of the family's entry point, decided on the host before any launch, in this
 * order: LTR_ERR_KIND (unknown family, loss code, label dtype or algo), LTR_ERR_SHAPE (the network and list limits of
 * the entry point, a sigma it refuses, w1_pitch outside [1, F], lr or weight_decay / momentum / eps / lr_decay negative
 * or not finite, nesterov without momentum or with dampening, betas outside [0, 1)), LTR_ERR_LIST_TOO_LONG; B == 0
 * is a no-op (nothing is launched: parameters, state and step count untouched); LTR_ERR_NULL (optim, X, a parameter,
 * rel, n, loss, a state the algorithm needs, W1_rows where w1_pitch < F), LTR_ERR_WORKSPACE, LTR_ERR_CONFIG (a
 * listwise or LambdaRank shape off its plan).
 */
int ltr_mlp_train_step_f32(int family, int code, int k, float sigma, const float *X, float *W1, float *b1, float *W2,
                           float *b2, float *W3, float *b3, int w1_pitch, const float *W1_rows, const void *rel,
                           int rel_dtype, const int64_t *n, const int32_t *tie, int use_seed, uint64_t seed,
                           const int64_t *seed_dev, const float *grad_out, int B, int L, int F, int H1, int H2,
                           float *loss, float *scores_out, float *loss_sum, float *state,
                           const struct ltr_mlp_optim *optim, float *grads_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/*
 * The same update as one elementwise launch (a block per 1024 parameters) on a flat gradient already summed -- the
 * `grads` of ltr_mlp_rows_grad_f32, ltr_mlp_wide_grad_f32 or ltr_mlp_bf16_grad, rows of F floats: parameters, w1_pitch
 * and state as above, and the same step count.  Errors: LTR_ERR_KIND (algo), LTR_ERR_SHAPE (F, H1, H2 <= 0, w1_pitch,
 * the hyper-parameters), LTR_ERR_NULL (optim, grads, a parameter, a state the algorithm needs).
 */
int ltr_mlp_apply_update_f32(const float *grads, float *W1, float *b1, float *W2, float *b2, float *W3, float *b3,
                             int w1_pitch, float *state, const struct ltr_mlp_optim *optim, int F, int H1, int H2,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MLP_TRAIN_H */
