/*
 * hnh_attn_additive.h — additive (a1, a2) attention scores for the GAT (GAT score "additive", csrc/host/gat.hpp), forward and backward,
 * exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h, include/hnh_attention.h and include/hnh_attn_grad.h: the host layer
 * binds it with dlsym and leaves it null when a kernel library does not export it (neither CPU test double under oracle/ does); the
 * additive score then fails with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h:
 * device pointers, row-major fp64, int status, asynchronous.
 *
 * Per head, with A = X W_h (rows x f), the head's slices a1, a2 (f entries each), g(z) = z > 0 ? 1 : alpha, over the nonzeros (i, j)
 * of S (a repeated pair counts as often as it appears):
 *     s_i = <A_i, a1>     t_j = <A_j, a2>     z_ij = s_i + t_j     e_ij = LeakyReLU_alpha(z_ij)
 *     lse_i = log sum_j exp(e_ij)     a_ij = exp(e_ij - lse_i)     o_i = sum_j a_ij A_j                     (forward)
 *     da_ij = <dZ_i, A_j>     dz_ij = a_ij (da_ij - delta_i) g(z_ij)     delta_i = <dZ_i, o_i>
 *     ds_i = sum_j dz_ij      dt_j = sum_i dz_ij      dAgg_j = sum_i a_ij dZ_i                              (backward)
 * No pass forms a dot product of two gathered rows' worth of data for the SCORE: it is one addition per nonzero.
 *
 * Two dense operands carry a row's scalars side by side with its vector, so that ONE gather per nonzero brings both (and a schedule
 * that moves exactly one dense operand between ranks moves everything a pass needs); fp = f rounded up to even:
 *
 *     scored operand   M_r = [ A_r[0 : f] (pad) | s_r t_r ]                 HNH_ATTN_ADD_SCORED_WIDTH(f) = fp + 2 doubles
 *     packed operand   Q_r = [ dZ_r[0 : f] (pad) | s_r lse_r delta_r 0 ]    HNH_ATTN_ADD_PACKED_WIDTH(f) = fp + 4 doubles
 *                              ^ column 0           ^ column fp
 *
 * The pad column (present when f is odd) holds zero.  Both are read at an even pitch from a 16-byte aligned base, so the scalars sit
 * on a 16-byte boundary whatever f is.  hnh_attn_add_scores_f64 builds M from A, hnh_attn_add_pack_f64 builds Q; these layouts are the
 * contract between them and the three passes.
 *
 * Widths: every f <= HNH_ATTN_ADD_MAX_F; 64, 128 and 256 run exact-width instances (16-byte aligned operands with even pitches),
 * every other width a bounds-checked one (8-byte lanes when f is odd or an operand is misaligned).  A wider head returns
 * HNH_ERR_UNSUPPORTED and writes nothing.  No atomics: every result is bit-identical run to run.
 */
#ifndef HNH_ATTN_ADDITIVE_H
#define HNH_ATTN_ADDITIVE_H
#include "hnh_attention.h" /* HNH_ATTN_FINISH */
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_ADD_MAX_F 256
#define HNH_ATTN_ADD_SCORED_WIDTH(f) ((f) + ((f) & 1) + 2)
#define HNH_ATTN_ADD_PACKED_WIDTH(f) ((f) + ((f) & 1) + 4)

typedef struct hnh_attn_add {
    const double* M;   /* scored operand of the block's OWN rows (s_i for the forward and the row pass; A_j and t_j for the column pass) */
    int64_t ld_m;      /* >= fp + 2 */
    const double* dZ;  /* row pass: dZ rows of the block's rows */
    int64_t ld_dz;
    double* lse;       /* forward: written by the finishing call (0 for a row without nonzeros); row pass: read (final) */
    const double* delta; /* row pass: delta_i */
    const double* Y;   /* the gathered operand: M of the block's columns (forward, row pass) or Q (column pass); even pitch, 16-byte aligned */
    int64_t ld_y;
    double* Out;       /* forward: the running accumulator, rows x f (undefined after the finishing call); column pass: dAgg, rows x f */
    int64_t ld_out;
    double* vec;       /* row pass: ds; column pass: dt; element r at vec[r * ld_vec] */
    int64_t ld_vec;
    double* row_max;   /* forward: the rows' running max and sum (the protocol of hnh_attn_softmax_csr_p) */
    double* row_sum;
    double* relu_dst;  /* forward: the finishing call writes act(o_i) to relu_dst[i * relu_ld + c], c < f (max(o_i, 0) unless an HNH_ATTN_ACT_* flag is set) */
    int64_t relu_ld;
    int f;             /* head width */
    double leaky_alpha;
} hnh_attn_add;

/* Forward pass over a block of S (or a window of it).  The row state (M, l, Out row) lives in row_max, row_sum and Out and a call
 * CONTINUES from it nonzero by nonzero, exactly as hnh_attn_softmax_csr_p does with s_u = LeakyReLU(s_i + t_j): results do not depend
 * on how a row's nonzeros are split into column panels, windows or groups of windows.  flags: HNH_FUSED_OUT_OVERWRITE (every row of the
 * call starts from the empty state), HNH_ATTN_FINISH (this call finishes the rows: ReLU(acc / l) into relu_dst, lse; the whole pass
 * or the window with `last` set), and with it HNH_ATTN_ACT_ELU or HNH_ATTN_ACT_IDENTITY (hnh_attention.h: the activation in ReLU's place) and HNH_ATTN_ADDEND (hnh_gat_skip.h: the addend that waits in relu_dst).  Hub rows are walked whole by one group.  b->rowptr == NULL: a block of b->rows rows without any
 * nonzero (the reset and the finish still apply). */
int hnh_attn_add_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream);

/* Backward row pass over a block of S:       vec_i (+)= sum_j dz_ij                                   (dZ_i, s_i, lse_i, delta_i in registers)
 * Backward column pass over a block of S^T:  Out_j (+)= sum_i a_ij Q_i[0 : f],  vec_j (+)= sum_i dz_ij   (A_j, t_j in registers; nonzero (j, i) = S_ij)
 * flags: HNH_FUSED_OUT_OVERWRITE or 0.  Both add their nonzeros to the loaded value in row order; hub rows (hnh_kernels.h) take
 * 256-nonzero segments into partial results which are added up in segment order with the pass's last call, so a row's result does not
 * depend on how it is split into panels, windows or groups of windows.  b->rowptr == NULL: no nonzeros (overwrite stores zeros). */
int hnh_attn_add_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream);
int hnh_attn_add_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream);

/* M[r, :] = [A[r, 0 : f] (0) | <A_r, a1> <A_r, a2>] for r < rows: one read of A.  ld_m even and >= fp + 2; M must not alias A. */
int hnh_attn_add_scores_f64(hnh_ctx* ctx, double* M, int64_t ld_m, const double* A, int64_t ld_a, const double* a1, const double* a2,
                            int64_t rows, int f, int stream);

/* Q[r, :] = [dZ[r, 0 : f] (0) | M[r, fp] lse[r] delta[r] 0] for r < rows.  ld_q even and >= fp + 4. */
int hnh_attn_add_pack_f64(hnh_ctx* ctx, double* Q, int64_t ld_q, const double* dZ, int64_t ld_dz, const double* M, int64_t ld_m,
                          const double* lse, const double* delta, int64_t rows, int f, int stream);

/* dA[r, col0 + c] = dAgg[r, c] + ds[r] a1[c] + dt[r] a2[c] for r < rows, c < f, with ds[r] = D[r * ld_d], dt[r] = D[r * ld_d + 1]. */
int hnh_attn_add_update_f64(hnh_ctx* ctx, double* dA, int64_t ld_da, int64_t col0, const double* dAgg, int64_t ld_g, const double* D,
                            int64_t ld_d, const double* a1, const double* a2, int64_t rows, int f, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_ADDITIVE_H */
