/* neupan_amd_train.h -- C ABI of the fused DUNE training step (libneupan_amd_train.so).
 *
 * A second library next to libneupan_amd.so (include/neupan_amd.h), with this header as its specification: the
 * optimisation of `DUNETrain` (neupan/blocks/dune_train.py:302-366: forward, four losses, backward, Adam) for the
 * ObsPointNet 2 -> 32 -> 32 -> 32 -> 32 -> 32 -> E, as ONE kernel launch per series of steps.  The conventions are
 * neupan_amd.h's: int status (0 = ok, < 0 = NPA_E_*), device pointers owned by the caller, `stream` a hipStream_t
 * passed as void*, nothing synchronises, fp32 C-contiguous arrays.
 *
 * Parameter pack (P = 4512 + 33 E floats per run): the state_dict order of ObsPointNet, every tensor row-major, so a
 * pack is the flat concatenation of the state_dict's tensors.  Offsets in floats:
 *        0  MLP.0.weight  [32,2]      64  MLP.0.bias  [32]      96  MLP.1.weight [32]    128  MLP.1.bias [32]   (LayerNorm)
 *      160  MLP.3.weight  [32,32]   1184  MLP.3.bias  [32]
 *     1216  MLP.5.weight  [32,32]   2240  MLP.5.bias  [32]    2272  MLP.6.weight [32]   2304  MLP.6.bias [32]   (LayerNorm)
 *     2336  MLP.8.weight  [32,32]   3360  MLP.8.bias  [32]
 *     3392  MLP.10.weight [32,32]   4416  MLP.10.bias [32]    4448  MLP.11.weight [32]  4480  MLP.11.bias [32]  (LayerNorm)
 *     4512  MLP.13.weight [E,32]    4512 + 32 E  MLP.13.bias [E]
 *
 * Network (obs_point_net.py:31-46): three times Linear -> LayerNorm(eps 1e-5, biased variance) -> tanh -> Linear -> ReLU;
 * the last Linear has width E, mu = its ReLU.
 *
 * Losses of one batch of b rows (dune_train.py:302-366), p the point, mu_l / d_l the labels, (c, s) = rot[step]:
 *     dist = sum_e mu_e (G p - h)_e                           R = [[c, -s], [s, c]],  M = -R G^T  (2 x E)
 *     fa = M mu,  fb = fa . p + mu . h                        fa_l, fb_l: the same with mu_l
 *     losses[0] = sum (mu - mu_l)^2 / (b E)    losses[1] = sum (dist - d_l)^2 / b
 *     losses[2] = sum (fa - fa_l)^2 / (2 b)    losses[3] = sum (fb - fb_l)^2 / b          total = their sum
 *
 * Adam (torch.optim.Adam, no amsgrad), t = step_count + 1 for the step at hand, g the gradient of the total:
 *     g += weight_decay p;   m += (1 - beta1) (g - m);   v = beta2 v + (1 - beta2) g g
 *     p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * Each line is one fused multiply-add (the product (1 - beta2)(g g) with g g rounded first), sqrt and the two divisions are
 * correctly rounded: the roundings of torch's foreach kernels, so the parameters are torch.optim.Adam's to the bit.
 * lr, beta1 and beta2 arrive as floats and are taken as the decimal numbers they were written as: each is rounded to
 * 7 significant digits in double (0.9f -> 0.9, 0.999f -> 0.999) before 1 - beta and the bias corrections (double,
 * beta^t = exp(t log beta), rounded to float once) are formed, which is what torch computes from its python floats.
 *
 * Order of every sum (the results are a function of the inputs alone: no atomics, no dependence on timing, on `runs`
 * or on how a series of steps is split over launches):
 *   - one workgroup of 256 threads per run; a step's batch is taken in chunks of 256 rows, one row per thread;
 *   - a dot product over a layer's inputs is one fmaf chain over k = 0 .. 31 starting from the bias (forward) or from
 *     zero over the outputs j = 0 .. 31 (backward);
 *   - an element of a weight or bias gradient is one chain over the chunk's rows in ascending order, chunks added in
 *     ascending order; a LayerNorm weight or bias gradient sums rows r = 4 q + 32 i + {0,1,2,3} (i ascending) in eight
 *     partial sums q = 0 .. 7 and then adds them pairwise (q ^ 1, q ^ 2, q ^ 4);
 *   - a loss term sums per row over e, then over the 64 lanes of a wave pairwise (lane ^ 32, 16, .. 1), then the four
 *     waves in ascending order, then the chunks in ascending order.
 */
#ifndef NEUPAN_AMD_TRAIN_H
#define NEUPAN_AMD_TRAIN_H

#include "neupan_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the exports of the library: everything else in it is built with hidden visibility */
#pragma GCC visibility push(default)

/* P = 4512 + 33 * edge_num.  Host only.  NPA_E_ARG (< 0) for edge_num outside 3 .. NPA_MAX_E. */
int npa_dune_train_param_count(int edge_num);

/* `steps` consecutive optimisation steps (train != 0) or loss evaluations (train == 0) of `runs` independent runs, one
 * launch.  Step s uses rows [first_row + s * batch, min(that + batch, n)) of every run's data set: the last batch may be
 * short, an empty one is refused.
 *   G [runs,E,2], h [runs,E]                       the robots' half-planes G x <= h
 *   points [runs,n,2], mu [runs,n,E], dist [runs,n]  the data set: points and their labels
 *   rot [steps,2]                                  cos and sin of each step's rotation angle (shared by the runs)
 *   params, adam_m, adam_v [runs,P], step_count [runs]   the state: read, and with train != 0 written (step_count += steps)
 *   losses [runs,steps,4]                          mu, distance, fa, fb loss of each step's batch, BEFORE that step's update
 *   grad_out [runs,P] or NULL                      train != 0 only: gradient of the total loss of the LAST step, before
 *                                                  weight decay
 * train == 0 writes nothing but `losses`; adam_m, adam_v, step_count and grad_out are not touched and may be NULL.
 * All state between launches is in params, adam_m, adam_v and step_count: n steps in one launch and the same steps over
 * several launches (first_row and rot advanced) give the same bits.
 * NPA_E_ARG (before anything touches a device): runs < 1, batch < 1, steps < 1, n < 1, first_row < 0, an empty step
 * (first_row + (steps - 1) * batch >= n), edge_num outside 3 .. NPA_MAX_E, a NULL required pointer. */
int npa_dune_train_steps(int runs, int edge_num, const float *G, const float *h, int64_t n, const float *points,
                         const float *mu, const float *dist, int64_t first_row, int batch, int steps, const float *rot,
                         float lr, float beta1, float beta2, float eps, float weight_decay, int train, float *params,
                         float *adam_m, float *adam_v, int32_t *step_count, float *losses, float *grad_out, void *stream);

/* message of the calling thread's last failed call of this library */
const char *npa_dune_train_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
