/*
 * hnh_attention.h — neighbourhood-softmax attention for the GAT (GAT attention mode "softmax", csrc/host/gat.hpp), exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (the plain CPU test double, oracle/liboracle_backend.so, does not; the second one, oracle/liboracle_backend_gat.so, does); the softmax mode then fails with an error naming the
 * missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status,
 * asynchronous.
 *
 * Per row i of a block, over its nonzeros (i, j) in row order (a repeated pair counts as often as it appears):
 *     s_ij = LeakyReLU_alpha(<X_i, Y_j>)
 *     M    = max_j s_ij,   l = sum_j exp(s_ij - M),   lse_i = M + log l,   o_i = sum_j exp(s_ij - lse_i) Y_j
 * The row's running state (M, l, Out row) lives in row_max[i], row_sum[i] and Out[i, :].  A call CONTINUES from it, nonzero by
 * nonzero:
 *     M_u = max(M_{u-1}, s_u);   f = exp(M_{u-1} - M_u) (1 when the max does not rise, 0 from the empty state)
 *     Out = Out * f + exp(s_u - M_u) Y_u;   l = l * f + exp(s_u - M_u)
 * so the result does not depend on how a row's nonzeros are split into calls (column panels, windows, groups of windows).
 */
#ifndef HNH_ATTENTION_H
#define HNH_ATTENTION_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

/* flag of hnh_attn_softmax_csr_p besides HNH_FUSED_VALUES_OVERWRITE / HNH_FUSED_OUT_OVERWRITE: this call finishes the rows (the
 * whole pass, or the window with `last` set).  HNH_FUSED_OUT_OVERWRITE starts every row of the call from the empty state
 * (M = -inf, l = 0, Out row = 0), whether the row has nonzeros in the call or not. */
#define HNH_ATTN_FINISH 8u
/* Output activation of the finishing call, with o_i the finished row (o_i = 0 without nonzeros): neither bit writes max(o_i, 0) (ReLU),
 * HNH_ATTN_ACT_ELU writes o for o > 0 and expm1(o) otherwise, HNH_ATTN_ACT_IDENTITY writes o_i itself.  Meaningful only together with
 * HNH_ATTN_FINISH: both bits at once, or one without HNH_ATTN_FINISH, return HNH_ERR_INVALID and write nothing.  The same bits serve
 * hnh_attn_add_fwd_csr_p (hnh_attn_additive.h) and hnh_attn_drop_fwd_csr_p (hnh_attn_dropout.h).  A library that exports
 * hnh_act_grad_cols_f64 (hnh_grad.h) knows them.  (A further public bit of the finishing call, HNH_ATTN_ADDEND = 0x40: hnh_gat_skip.h.) */
#define HNH_ATTN_ACT_ELU 0x10u
#define HNH_ATTN_ACT_IDENTITY 0x20u

typedef struct hnh_attn_state {
    double* row_max;    /* rows: running max M */
    double* row_sum;    /* rows: running sum l */
    double* lse;        /* rows: M + log l, written by the finishing call (0 for a row without nonzeros) */
    double leaky_alpha; /* slope of the LeakyReLU applied to the scores */
    double* relu_dst;   /* the finishing call writes act(o_i) to relu_dst[i * relu_ld + c], c < R: max(o_i, 0) unless an HNH_ATTN_ACT_* flag is set */
    int64_t relu_ld;
} hnh_attn_state;

/* One softmax-attention pass over a block (or a window of it), X = the row operand, Y = the gathered operand (R columns each),
 * Out = the running accumulator (rows x R; undefined after the finishing call).  values[e] receives s_e (the activated score).
 * b->rowptr == NULL: a block of b->rows rows without any nonzero (the flags' state reset and the finish still apply).
 * Widths: one pass over the row's R columns.  R in {64, 128, 256} run exact-width instances and every other R <= 512 a bounds-checked
 * one, but an R above 256 only when R is even, X, Y, Out and state->relu_dst are 16-byte aligned and state->relu_ld is even (the
 * 16-byte instances); otherwise R <= 256.  Wider rows return HNH_ERR_UNSUPPORTED and write nothing.  A block without nonzeros
 * (rowptr == NULL) takes any R.  Hub rows are walked whole by one group, never split (bit-identical results at any grouping). */
int hnh_attn_softmax_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, double* values, const double* X, const double* Y, double* Out, int R,
                           unsigned flags, const hnh_attn_state* state, const hnh_csr_window* window, int stream);

/* Backward gate, in place over n nonzeros, with lse and delta broadcast onto the nonzeros:
 *     a  = exp(LeakyReLU_alpha(e) - lse)                      e -> a
 *     de = a * (da - delta) * (e > 0 ? 1 : alpha)            da -> de */
int hnh_softmax_gate_f64(hnh_ctx* ctx, double* e_to_a, double* da_to_de, const double* lse, const double* delta, double alpha, int64_t n,
                         int stream);

/* out[r] = <dZ[r, 0 : cols], O[r, col0 : col0 + cols]> for r < rows (delta_i = <dZ_i, o_i> of the backward pass). */
int hnh_rowdot_cols_f64(hnh_ctx* ctx, double* out, const double* dZ, int64_t ld_dz, const double* O, int64_t ld_o, int64_t col0, int64_t rows,
                        int64_t cols, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTENTION_H */
