/*
 * hnh_attn_v2.h — GATv2 dynamic attention scores for the GAT (GAT score "gatv2", csrc/host/gat.hpp), forward and backward, exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_attn_grad.h and include/hnh_attn_additive.h: the host layer binds it with dlsym
 * and leaves it null when a kernel library does not export it (neither CPU test double under oracle/ does); the gatv2 score then fails
 * with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major
 * fp64, int status, asynchronous.
 *
 * Per head, with A = X W_h (rows x f), the head's vector a (f entries), alpha the LeakyReLU slope, over the nonzeros (i, j) of S (a
 * repeated pair counts as often as it appears) (Brody, Alon, Yahav: the nonlinearity sits INSIDE the contraction):
 *     u_ijc = A_ic + A_jc     sg_ijc = u_ijc > 0 ? 1 : alpha     z_ij = sum_c a_c sg_ijc u_ijc     (no outer LeakyReLU)
 *     lse_i = log sum_j exp(z_ij)     p_ij = exp(z_ij - lse_i)     o_i = sum_j p_ij A_j                     (forward)
 *     g_ij = p_ij (<dZ_i, A_j> - delta_i)     delta_i = <dZ_i, o_i>
 *     R_ic = sum_j g_ij sg_ijc     C_jc = sum_i g_ij sg_ijc     dAgg_j = sum_i p_ij dZ_i                   (backward)
 *     T = R + C     dA = dAgg + T o a     da_c = sum_r A_rc T_rc
 * The last line holds because LReLU(u) = sg (A_ic + A_jc): sum_ij g sg u splits into the row side and the column side, so the gradient
 * of a needs no sparse work of its own.
 *
 * The forward pass and the row pass gather A_j (f doubles per nonzero, what hnh_attn_softmax_csr_p gathers); the column pass over S^T
 * gathers the packed operand P_i = [A_i (0) | dZ_i (0) | lse_i delta_i] of include/hnh_attn_grad.h, built by hnh_attn_grad_pack_f64 with
 * lse and delta: that layout is used unchanged (HNH_ATTN_GRAD_PACKED_WIDTH(f, 1) doubles, an even pitch, a 16-byte aligned base).
 *
 * Widths: every f <= HNH_ATTN_V2_MAX_F; 64, 128 and 256 run exact-width instances (16-byte aligned operands with even pitches), every
 * other width a bounds-checked one (8-byte lanes when f is odd or an operand is misaligned): the rules of hnh_attn_grad.h.  A wider head
 * returns HNH_ERR_UNSUPPORTED and writes nothing.  No atomics: every result is bit-identical run to run.
 */
#ifndef HNH_ATTN_V2_H
#define HNH_ATTN_V2_H
#include "hnh_attention.h" /* HNH_ATTN_FINISH, HNH_ATTN_ACT_* */
#include "hnh_attn_grad.h" /* the packed operand of the column pass */
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_V2_MAX_F 256
/* doubles of workspace that hnh_attn_v2_finish_f64 needs for a head of f features (1024 partial rows of da) */
#define HNH_ATTN_V2_FINISH_WORK(f) (1024 * (int64_t)(f))

typedef struct hnh_attn_v2 {   /* 152 bytes: seventeen pointers and pitches, an int (padded), a double */
    const double* X;    /* the block's OWN rows of A (all three passes) */
    int64_t ld_x;
    const double* a;    /* the head's vector, f entries */
    const double* dZ;   /* row pass: dZ rows of the block's rows */
    int64_t ld_dz;
    double* lse;        /* forward: written by the finishing call (0 for a row without nonzeros); row pass: read (final) */
    const double* delta; /* row pass: delta_i */
    const double* Y;    /* the gathered operand: A of the block's columns (forward, row pass; ld_y >= f) or the packed P (column pass) */
    int64_t ld_y;
    double* Out;        /* forward: the running accumulator (undefined after the finishing call); row pass: R; column pass: C; rows x f */
    int64_t ld_out;
    double* Out2;       /* column pass: dAgg, rows x f */
    int64_t ld_out2;
    double* row_max;    /* forward: the rows' running max and sum (the protocol of hnh_attn_softmax_csr_p) */
    double* row_sum;
    double* relu_dst;   /* forward: the finishing call writes act(o_i) to relu_dst[i * relu_ld + c], c < f (max(o_i, 0) unless an HNH_ATTN_ACT_* flag is set) */
    int64_t relu_ld;
    int f;              /* head width */
    double leaky_alpha;
} hnh_attn_v2;

/* Forward pass over a block of S (or a window of it).  The row state (M, l, Out row) lives in row_max, row_sum and Out and a call
 * CONTINUES from it nonzero by nonzero, exactly as hnh_attn_softmax_csr_p does with s_u = z_ij: results do not depend on how a row's
 * nonzeros are split into column panels, windows or groups of windows.  flags: HNH_FUSED_OUT_OVERWRITE (every row of the call starts from
 * the empty state), HNH_ATTN_FINISH (this call finishes the rows: act(acc / l) into relu_dst, lse; the whole pass or the window with
 * `last` set), and with it HNH_ATTN_ACT_ELU or HNH_ATTN_ACT_IDENTITY and HNH_ATTN_ADDEND (hnh_gat_skip.h: the addend that waits in relu_dst).  Hub rows are walked whole by one group.  b->rowptr == NULL: a
 * block of b->rows rows without any nonzero (the reset and the finish still apply). */
int hnh_attn_v2_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_v2* args, unsigned flags, const hnh_csr_window* window,
                          int stream);

/* Backward row pass over a block of S:       Out_i (+)= sum_j g_ij sg_ij                     (A_i, dZ_i, lse_i, delta_i, a in registers; gathers A_j)
 * Backward column pass over a block of S^T:  Out_j (+)= sum_i g_ij sg_ij,  Out2_j (+)= sum_i p_ij dZ_i   (A_j, a in registers; gathers P_i;
 *                                            nonzero (j, i) = S_ij).  Two accumulators per row go to two outputs.
 * flags: HNH_FUSED_OUT_OVERWRITE or 0.  Both add their nonzeros to the loaded value in row order; hub rows (hnh_kernels.h) take
 * 256-nonzero segments into partial rows which are added up in segment order with the pass's last call, so a row's result does not
 * depend on how it is split into panels, windows or groups of windows.  b->rowptr == NULL: no nonzeros (overwrite stores zeros). */
int hnh_attn_v2_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_v2* args, unsigned flags, const hnh_csr_window* window,
                          int stream);
int hnh_attn_v2_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_v2* args, unsigned flags, const hnh_csr_window* window,
                          int stream);

/* One dense pass per head: with T = Rm + Cm,  dA[r, col0 + c] = dAgg[r, c] + T[r, c] a[c]  and  da[c * ld_dav] = sum_r A[r, c] T[r, c]
 * for r < rows, c < f.  The workgroups' partial column sums go to `work` (at least HNH_ATTN_V2_FINISH_WORK(f) doubles) and are added in
 * a fixed order: bit-identical run to run, no atomics.  rows == 0 stores da = 0. */
int hnh_attn_v2_finish_f64(hnh_ctx* ctx, double* dA, int64_t ld_da, int64_t col0, const double* dAgg, int64_t ld_g, const double* Rm,
                           int64_t ld_r, const double* Cm, int64_t ld_c, const double* A, int64_t ld_a, const double* a, double* da,
                           int64_t ld_dav, int64_t rows, int f, double* work, int64_t work_doubles, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_V2_H */
