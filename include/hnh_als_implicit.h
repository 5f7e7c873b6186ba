/*
 * hnh_als_implicit.h — the dense half of one CG iteration of implicit-feedback ALS (Implicit_ALS in csrc/host/als_implicit.hpp): the
 * Gram term of the half-step's operator, M(p)_i = sum_e w_e <p_i, y_j> y_j + lambda p_i + p_i G with G = Y^T Y, added to the fused
 * SDDMM -> SpMM call's output, and the guarded CG update of the row while it is on chip.  Exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_train_clip.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); Implicit_ALS in folded mode then fails with an error naming
 * the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status,
 * asynchronous on the given stream.  No atomics and every reduction in a fixed order: every result is bit-identical run to run.
 */
#ifndef HNH_ALS_IMPLICIT_H
#define HNH_ALS_IMPLICIT_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The widest row hnh_gram_rows_f64 takes: the whole output row of a row tile stays in the accumulators of one wave. */
#define HNH_GRAM_MAX_R 256

/* The CG state of the rows, updated in place (all rows x R but rs, which has one entry per row). */
typedef struct hnh_gram_cg {
    double* x;  /* the factor being optimised */
    double* r;  /* residual */
    double* p;  /* search direction = the call's X */
    double* rs; /* <r, r> of the previous iteration in, of this one out */
} hnh_gram_cg;

/* Mp[i,:] = Out[i,:] + X[i,:] * G for i < rows, with G row-major R x R and Out what the fused call left there (sum_e w_e <x_i, y_j> y_j
 * + lambda x_i).  A rows x R by R x R product on the fp64 matrix cores whose output tile is the whole row, with a row-wise epilogue:
 *   cg == NULL: Mp is stored to Out; rowdot != NULL: rowdot[i] = <X[i,:], Mp[i,:]>.
 *   cg != NULL: cg->p must be X (writable) and rowdot is ignored.  The guarded CG update runs on the row:
 *       bdot  = <p_i, Mp>;                    live  = rs_i > 0 and bdot > 0;       alpha = live ? rs_i / bdot : 0
 *       x_i  += alpha p_i;                    r_i  -= alpha Mp;                    rsnew = <r_i, r_i>
 *       beta  = live ? rsnew / rs_i : 0;      p_i   = r_i + beta p_i;              rs_i  = rsnew
 *     There is no epsilon: a row that is not live keeps x_i and r_i bit for bit (they are not stored), and gets p_i = r_i.  Out is
 *     not written back.  Row i of p is read only by the wave that owns row i, so updating it in place is safe.
 * Any 1 <= R <= HNH_GRAM_MAX_R and any rows >= 0 (rows == 0: nothing is launched); remainders in rows and in R are handled.  A wider
 * R, a null pointer, or cg->p != X fail with HNH_ERR_INVALID and a message, and nothing is launched. */
int hnh_gram_rows_f64(hnh_ctx* ctx, double* Out, const double* X, const double* G, int64_t rows, int R, double* rowdot,
                      const hnh_gram_cg* cg, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ALS_IMPLICIT_H */
