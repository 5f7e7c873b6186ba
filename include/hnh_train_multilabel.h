/*
 * hnh_train_multilabel.h — the multi-label head of the GAT's training step (GAT::set_multilabel_targets in csrc/host/gat.hpp): a masked,
 * class-weighted sigmoid cross-entropy over the rows of the last layer's output, with the counts of micro-averaged F1.  Exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_train.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); loss / train_step / evaluate under the sigmoid head then fail
 * with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_train.h: device pointers, row-major fp64, int
 * status, asynchronous on the given stream.  No floating-point atomics: every result is bit-identical run to run.
 *
 * The loss.  A row r of `out` holds `heads` blocks of `classes` logits, as in hnh_xent_rows_f64.  For every row whose mask byte is not 0
 * and every class c, with y the target bit and w = pos_weight[c] (1 without weights):
 *     z    = (sum over h ascending of out[r, h * classes + c]) * (1 / heads)
 *     e    = exp(-|z|);   sp = log1p(e)
 *     loss = w y (max(-z, 0) + sp) + (1 - y) (max(z, 0) + sp)        = -w y log s(z) - (1 - y) log(1 - s(z)), finite for every finite z
 *     s    = z >= 0 ? 1 / (1 + e) : e / (1 + e)
 *     G[r, h * classes + c] = (inv_n / heads) (s (1 - y + w y) - w y)  for every h;  a row whose mask byte is 0 gets G = 0
 *     pred = z > 0                                                      (z == 0 predicts "absent")
 * (the y = 1 branch of G is evaluated as -(inv_n / heads) w (1 - s) with 1 - s from e, which does not cancel where s is close to 1).
 * A class needs nothing from the other classes of its row: no row is staged, and there is NO width limit (HNH_XENT_MAX_WIDTH does not
 * apply).  A lane reads its class's `heads` values and writes the same elements, so G may alias out.
 */
#ifndef HNH_TRAIN_MULTILABEL_H
#define HNH_TRAIN_MULTILABEL_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One pass over `out` (rows x heads * classes, pitch ld_out >= heads * classes): every row in the loss is read once and, when G is not
 * null, every row of G (pitch ld_g >= heads * classes) written once.
 * targets: bit-packed, bit (c % 32) of word c / 32 of row r's ld_t words; ld_t >= (classes + 31) / 32.  The bits beyond `classes` in a
 * row's last word are never read as classes.  row_mask: one byte per row.  pos_weight_or_null: `classes` doubles; null: every weight 1,
 * bit-identical to passing ones.
 * result[0] = the sum of `loss` over the rows in the loss and their classes, result[1] = tp, result[2] = fp, result[3] = fn: counts of
 * (row, class) pairs held as doubles, exact.  Reduced in a fixed order: one set of partials per workgroup in `work`, then one ordered
 * finishing launch.  `work` must hold hnh_bce_rows_f64_workspace(rows) doubles.  A NaN in a row of the loss makes result[0] NaN.
 * heads < 1, classes < 1, a pitch too small or a workspace too small fail with HNH_ERR_INVALID, and nothing is launched. */
int64_t hnh_bce_rows_f64_workspace(int64_t rows);
int hnh_bce_rows_f64(hnh_ctx* ctx, const double* out, int64_t ld_out, const uint32_t* targets, int64_t ld_t, const uint8_t* row_mask,
                     const double* pos_weight_or_null, int64_t rows, int heads, int classes, double inv_n, double* G_or_null, int64_t ld_g,
                     double* result, double* work, int64_t work_doubles, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_TRAIN_MULTILABEL_H */
