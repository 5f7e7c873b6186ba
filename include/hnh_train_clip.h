/*
 * hnh_train_clip.h — gradient clipping by global norm and decoupled weight decay for the GAT's training step (GAT::set_grad_clip and
 * optimizer kind AdamW in csrc/host/gat.hpp): the sum of squares of a table of gradient tensors, and the optimizer step of
 * include/hnh_train.h with a clip coefficient read from device memory.  Exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_train.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); optimizer_step / train_step with clipping switched on or with
 * kind AdamW then fail with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_train.h: device
 * pointers, row-major fp64, int status, asynchronous on the given stream; the table and the hyper-parameters are HOST memory, read before
 * the call returns.  No atomics: every result is bit-identical run to run.
 */
#ifndef HNH_TRAIN_CLIP_H
#define HNH_TRAIN_CLIP_H
#include "hnh_train.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Decoupled weight decay (torch.optim.AdamW): a third `kind` of struct hnh_optim, taken by hnh_optim_step_clip_f64 only. */
#define HNH_OPTIM_ADAMW 2
/* The most sums hnh_optim_step_clip_f64 adds up into the squared norm. */
#define HNH_CLIP_MAX_SUMS 8

/* result[0] (+)= sum over the n tensors k, in table order, of sum over r, c of g_k[r * ld_g + c]^2; accumulate != 0 adds onto the value
 * result[0] holds, to the bit: old + (what accumulate == 0 writes).  Of a table entry only g, ld_g, rows and cols are read; p, m and v
 * may be null.  A tensor without elements and an empty table (n == 0, tensors may then be null) give 0.
 * Two stages in a fixed order: every workgroup adds the squares of its share of ONE tensor into one partial in `work`, then one ordered
 * finishing launch adds the partials.  A table longer than HNH_OPTIM_MAX_TENSORS is split here into parts of that many, and the parts'
 * sums are added in table order.  The grid, the share of every thread and the order of every addition are functions of the table's rows,
 * cols and ld_g alone, never of the device or of where a tensor lies: 16-byte loads where base, pitch and width allow them and 8-byte
 * loads otherwise read the same elements into the same additions.  `work` must hold hnh_grad_sumsq_f64_workspace(tensors, n) doubles
 * (a negative value: the table is refused).
 * A null result, a short workspace, a negative shape, ld_g < cols, or a null g of a tensor with elements fail with HNH_ERR_INVALID, and
 * nothing is launched. */
int64_t hnh_grad_sumsq_f64_workspace(const hnh_optim_tensor* tensors, int n);
int hnh_grad_sumsq_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, int accumulate, double* result, double* work, int64_t work_doubles,
                       int stream);

/* hnh_optim_step_f64 (include/hnh_train.h: the same table, the same struct hnh_optim) with every gradient scaled by a clip coefficient
 * that every thread takes from device memory:
 *     coef = min(1, max_norm / (sqrt(sum over q < nsums of sumsq[q]) + 1e-6))        torch.nn.utils.clip_grad_norm_'s formula
 * and coef * g stands wherever hnh_optim_step_f64 has g.  sumsq == NULL: coef = 1 and nothing is read (nsums and max_norm are ignored).
 * A norm that is not finite gets NO special handling, which is clip_grad_norm_'s default (error_if_nonfinite=False): it propagates as
 * IEEE arithmetic has it, an infinite norm gives coef = 0 and a NaN norm a NaN coefficient and NaN parameters.
 * kind may also be HNH_OPTIM_ADAMW (bias1, bias2 as for Adam):
 *     p = p (1 - lr weight_decay);  then Adam's m, v and update of p with g' = coef * g, without the decay term      torch.optim.AdamW
 * On the bits: with coef == 1.0 (sumsq == NULL included) and kind Adam or SGD, p, m and v come out bit-identical to hnh_optim_step_f64's;
 * AdamW with weight_decay == 0 is bit-identical to Adam.
 * Fails like hnh_optim_step_f64, and with sumsq != NULL for nsums outside 1 .. HNH_CLIP_MAX_SUMS or a max_norm that is negative or NaN. */
int hnh_optim_step_clip_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, const hnh_optim* hyper, const double* sumsq, int nsums,
                            double max_norm, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_TRAIN_CLIP_H */
