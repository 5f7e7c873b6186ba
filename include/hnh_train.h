/*
 * hnh_train.h — the kernels of the GAT's training step (GAT::loss / optimizer_step / train_step in csrc/host/gat.hpp): a masked softmax
 * cross-entropy head over the rows of the last layer's output, and a table-driven optimizer over many parameter tensors.  Exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h, include/hnh_attention.h, include/hnh_attn_grad.h,
 * include/hnh_attn_additive.h and include/hnh_attn_dropout.h: the host layer binds it with dlsym and leaves it null when a kernel library
 * does not export it (the plain CPU test double, oracle/liboracle_backend.so, does not; the second one, oracle/liboracle_backend_gat.so, does); the training calls then fail with an error naming the missing symbol,
 * and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status, asynchronous on the given
 * stream.  No floating-point atomics: every result is bit-identical run to run.
 *
 * The loss.  A row r of `out` holds `heads` blocks of `classes` logits; with label l_r (a negative label: the row is not in the loss)
 *     z_c  = (1 / heads) * sum_h out[r, h * classes + c]         heads = 1: the "concat" reading; heads > 1: the mean over heads
 *     lp_c = z_c - max(z) - log(sum_c exp(z_c - max(z)))
 *     loss_sum = sum over labelled rows of -lp[l_r]
 *     correct  = number of labelled rows whose argmax_c z_c equals l_r (ties go to the lowest index)
 *     G[r, h * classes + c] = inv_n * (exp(lp_c) - [c == l_r]) / heads for labelled rows, 0 for the others
 * Known deviation from the published output layer: the heads arrive through the forward kernels' ReLU epilogue, so they are averaged
 * AFTER the ReLU; Velickovic et al. average the raw head outputs.
 */
#ifndef HNH_TRAIN_H
#define HNH_TRAIN_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The widest row hnh_xent_rows_f64 takes: heads * classes doubles (a row is staged once in a workgroup's LDS). */
#define HNH_XENT_MAX_WIDTH 4096

/* One pass over `out` (rows x heads * classes, pitch ld_out >= heads * classes): every row is read once and, when G is not null, its
 * row of G (pitch ld_g) written once.  result[0] = loss_sum, result[1] = correct, reduced in a fixed order: one set of partials per
 * workgroup in `work`, then one ordered finishing reduction.  `work` must hold hnh_xent_rows_f64_workspace(rows) doubles.
 * labels: one int32 per row.  A label >= classes is an error the device reports in the results (never an out-of-range read): the row is
 * treated as unlabelled, result[0] becomes NaN and result[1] minus the number of such rows.
 * heads * classes > HNH_XENT_MAX_WIDTH fails with HNH_ERR_INVALID.  G may alias out (a row is read before it is written). */
int64_t hnh_xent_rows_f64_workspace(int64_t rows);
int hnh_xent_rows_f64(hnh_ctx* ctx, const double* out, int64_t ld_out, const int32_t* labels, int64_t rows, int heads, int classes,
                      double inv_n, double* G, int64_t ld_g, double* result, double* work, int64_t work_doubles, int stream);

#define HNH_OPTIM_ADAM 0
#define HNH_OPTIM_SGD 1
/* Tensors one launch of hnh_optim_step_f64 takes (its table travels as kernel arguments); the entry point splits longer tables itself. */
#define HNH_OPTIM_MAX_TENSORS 32

/* One parameter tensor of rows x cols: p with pitch ld_p, its gradient g with pitch ld_g (a column block of a wider matrix, or one of
 * two interleaved vectors at pitch 2), and its moments m, v stored densely (pitch cols).  m is unused by SGD and may then be null. */
typedef struct hnh_optim_tensor {
    double* p;
    int64_t ld_p;
    const double* g;
    int64_t ld_g;
    double* m;
    double* v;
    int64_t rows, cols;
} hnh_optim_tensor;

typedef struct hnh_optim {
    int kind; /* HNH_OPTIM_ADAM | HNH_OPTIM_SGD */
    int reserved;
    double lr, beta1, beta2, eps, momentum, weight_decay;
    double bias1, bias2; /* 1 - beta1^t and 1 - beta2^t of this step, computed on the host in double */
} hnh_optim;

/* One step over n tensors (`tensors` and `hyper` are HOST memory, read before the call returns).  Per element, with g' = g + weight_decay * p:
 *     ADAM   m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g' g';  p -= lr (m / bias1) / (sqrt(v / bias2) + eps)
 *     SGD    v = momentum v + g';  p -= lr v
 * Tensors must not overlap. */
int hnh_optim_step_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, const hnh_optim* hyper, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_TRAIN_H */
