/*
 * hnh_attn_qkv.h — scaled dot-product attention with separate query, key and value projections for the GAT (GAT score "transformer",
 * csrc/host/gat.hpp), forward and backward, exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_attn_grad.h and include/hnh_attn_v2.h: the host layer binds it with dlsym and
 * leaves it null when a kernel library does not export it (neither CPU test double under oracle/ does); the transformer score then
 * fails with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major
 * fp64, int status, asynchronous.
 *
 * Per head, with Q = X W_q, K = X W_k, V = X W_v (rows x f each), scale = 1 / sqrt(f) handed in by the caller, over the nonzeros (i, j)
 * of S (a repeated pair counts as often as it appears; no LeakyReLU anywhere):
 *     s_ij = scale <Q_i, K_j>     lse_i = log sum_j exp(s_ij)     p_ij = exp(s_ij - lse_i)     o_i = sum_j p_ij V_j          (forward)
 *     delta_i = <dZ_i, o_i>       g_ij = scale p_ij (<dZ_i, V_j> - delta_i)
 *     dQ_i = sum_j g_ij K_j       dK_j = sum_i g_ij Q_i           dV_j = sum_i p_ij dZ_i                                     (backward)
 *
 * Every pass gathers ONE two-half packed row per nonzero, built by hnh_attn_grad_pack_f64 in the layout of include/hnh_attn_grad.h, which
 * is used unchanged (an even pitch, a 16-byte aligned base, fp = f rounded up to even, the pad column zero):
 *     forward and row pass:  [K_j (0) | V_j (0)]                       the pack with A = K, dZ = V, no scalars: HNH_ATTN_GRAD_PACKED_WIDTH(f, 0)
 *     column pass over S^T:  [Q_i (0) | dZ_i (0) | lse_i delta_i]      the pack with the softmax scalars:       HNH_ATTN_GRAD_PACKED_WIDTH(f, 1)
 * The dot product takes the first half; the forward pass's axpy takes the second.
 *
 * Widths: every f <= HNH_ATTN_QKV_MAX_F; 64, 128 and 256 run exact-width instances (16-byte aligned operands with even pitches), every
 * other width a bounds-checked one (8-byte lanes when f is odd or an operand is misaligned): the rules of hnh_attn_grad.h.  A wider head
 * returns HNH_ERR_UNSUPPORTED and writes nothing.  No atomics: every result is bit-identical run to run.
 */
#ifndef HNH_ATTN_QKV_H
#define HNH_ATTN_QKV_H
#include "hnh_attention.h" /* HNH_ATTN_FINISH, HNH_ATTN_ACT_* */
#include "hnh_attn_grad.h" /* the packed operands */
#include "hnh_gat_skip.h"  /* HNH_ATTN_ADDEND */
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_QKV_MAX_F 256

typedef struct hnh_attn_qkv {  /* 168 bytes: nineteen pointers and pitches, an int (padded), a double */
    const double* X;     /* the block's OWN rows: Q (forward, row pass) or K (column pass) */
    int64_t ld_x;
    const double* X2;    /* column pass: the block's own rows of V */
    int64_t ld_x2;
    const double* dZ;    /* row pass: dZ rows of the block's rows */
    int64_t ld_dz;
    double* lse;         /* forward: written by the finishing call (0 for a row without nonzeros); row pass: read (final) */
    const double* delta; /* row pass: delta_i */
    const double* Y;     /* the gathered packed operand (see above); ld_y even and at least the packed width */
    int64_t ld_y;
    double* Out;         /* forward: the running accumulator (undefined after the finishing call); row pass: dQ; column pass: dK; rows x f */
    int64_t ld_out;
    double* Out2;        /* column pass: dV, rows x f */
    int64_t ld_out2;
    double* row_max;     /* forward: the rows' running max and sum (the protocol of hnh_attn_softmax_csr_p) */
    double* row_sum;
    double* relu_dst;    /* forward: the finishing call writes act(o_i (+ addend)) to relu_dst[i * relu_ld + c], c < f */
    int64_t relu_ld;
    double* values;      /* forward, optional: values[e] receives s_e for every nonzero e of the call (block numbering) */
    int f;               /* head width */
    double scale;        /* the score's factor, 1 / sqrt(f) in the GAT */
} hnh_attn_qkv;

/* Forward pass over a block of S (or a window of it).  The row state (M, l, Out row) lives in row_max, row_sum and Out and a call
 * CONTINUES from it nonzero by nonzero, exactly as hnh_attn_softmax_csr_p does with s_u = s_ij: results do not depend on how a row's
 * nonzeros are split into column panels, windows or groups of windows.  flags: HNH_FUSED_OUT_OVERWRITE (every row of the call starts from
 * the empty state), HNH_ATTN_FINISH (this call finishes the rows: act(acc / l) into relu_dst, lse; the whole pass or the window with
 * `last` set), and with it HNH_ATTN_ACT_ELU or HNH_ATTN_ACT_IDENTITY and HNH_ATTN_ADDEND (hnh_gat_skip.h: the addend that waits in
 * relu_dst).  Hub rows are walked whole by one group.  b->rowptr == NULL: a block of b->rows rows without any nonzero (the reset and the
 * finish still apply). */
int hnh_attn_qkv_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window,
                           int stream);

/* Backward row pass over a block of S:       Out_i (+)= sum_j g_ij K_j                             (Q_i, dZ_i, lse_i, delta_i in registers; gathers [K_j | V_j])
 * Backward column pass over a block of S^T:  Out_j (+)= sum_i g_ij Q_i,  Out2_j (+)= sum_i p_ij dZ_i   (K_j, V_j in registers; gathers
 *                                            [Q_i | dZ_i | lse_i delta_i]; nonzero (j, i) = S_ij).  Two accumulators per row go to two outputs.
 * flags: HNH_FUSED_OUT_OVERWRITE or 0.  Both add their nonzeros to the loaded value in row order; hub rows (hnh_kernels.h) take
 * 256-nonzero segments into partial rows which are added up in segment order with the pass's last call, so a row's result does not
 * depend on how it is split into panels, windows or groups of windows.  b->rowptr == NULL: no nonzeros (overwrite stores zeros). */
int hnh_attn_qkv_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window,
                           int stream);
int hnh_attn_qkv_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window,
                           int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_QKV_H */
