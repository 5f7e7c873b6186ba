/*
 * hnh_attn_grad.h — the fused backward pass of the GAT's attention (GAT backward mode "fused", csrc/host/gat.hpp), exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h and include/hnh_attention.h: the host layer binds it with dlsym and
 * leaves it null when a kernel library does not export it (the plain CPU test double, oracle/liboracle_backend.so, does not; the second one, oracle/liboracle_backend_gat.so, does); the fused backward mode then
 * fails with an error naming the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers,
 * row-major fp64, int status, asynchronous.
 *
 * Per head, with A = X W_h, dZ = dL/d(pre-ReLU head output), g(e) = e > 0 ? 1 : alpha, over the nonzeros (i, j) of S (a repeated pair
 * counts as often as it appears):
 *     e_ij = <A_i, A_j>        da_ij = <dZ_i, A_j>
 *     attention none:      a_ij = LeakyReLU_alpha(e_ij)                  de_ij = da_ij g(e_ij)
 *     attention softmax:   a_ij = exp(LeakyReLU_alpha(e_ij) - lse_i)     de_ij = a_ij (da_ij - delta_i) g(e_ij)
 *     dA_i = sum_j de_ij A_j  +  sum_k (a_ki dZ_k + de_ki A_k)
 * The first sum is the ROW pass over a block of S (row i is the launch's own row: A_i, dZ_i, lse_i, delta_i sit in registers and one
 * gather of A_j serves both dot products and the axpy).  The second is the COLUMN pass over a block of S^T (row j of S^T is local, its
 * nonzero (j, i) stands for S_ij): everything that belongs to the gathered row i travels side by side in the PACKED operand
 *
 *     P_i = [ A_i[0 : f] (pad) | dZ_i[0 : f] (pad) | lse_i delta_i ]          hnh_attn_grad_packed_width(f, softmax) doubles
 *            ^ column 0          ^ column fp          ^ column 2 fp            fp = f rounded up to even
 *
 * The pad column (present when f is odd) holds zero, so the dZ half and the two scalars start on 16-byte boundaries of a row whose
 * pitch ld_p is even; the two scalars are absent for attention none.  One gather of P_i then gives e = <A_j, P_i[0 : f]>,
 * da = <A_j, P_i[fp : fp + f]>, the gate scalars, and both axpys into one accumulator: Out_j += a P_i[fp : fp + f] + de P_i[0 : f].
 * This layout is the contract between hnh_attn_grad_pack_f64 and hnh_attn_grad_col_csr_p.
 *
 * Both passes accumulate into Out as the fused SDDMM+SpMM pass does: a launch loads the output row, adds its nonzeros in row order
 * and stores it; HNH_FUSED_OUT_OVERWRITE starts from zero (rows without nonzeros then store zeros).  A row's result therefore does not
 * depend on how its nonzeros are split into column panels, windows or groups of windows, and it is bit-identical run to run (no
 * atomics).  Hub rows (hnh_kernels.h, the _ex entry points) take the segment path: 256-nonzero segments into partial rows, added up
 * in segment order.  Widths: every f <= HNH_ATTN_GRAD_MAX_F; 64, 128 and 256 run exact-width instances (16-byte aligned operands with
 * even pitches), every other width a bounds-checked one.  A wider head returns HNH_ERR_UNSUPPORTED and writes nothing.
 */
#ifndef HNH_ATTN_GRAD_H
#define HNH_ATTN_GRAD_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_GRAD_MAX_F 256

/* columns of a packed row (without any extra pitch): 2 fp, + 2 with softmax; always even */
#define HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax) (2 * ((f) + ((f) & 1)) + ((softmax) ? 2 : 0))

typedef struct hnh_attn_grad {
    const double* X;    /* row operand: A rows of the block's rows (both passes) */
    int64_t ld_x;
    const double* dZ;   /* row pass: dZ rows of the block's rows; column pass: unused */
    int64_t ld_dz;
    const double* lse;  /* row pass with softmax: lse_i and delta_i of the block's rows (both NULL: attention none); column pass: unused */
    const double* delta;
    const double* Y;    /* the gathered operand: A (row pass, ld_y >= f) or the packed P (column pass, ld_y >= the packed width, even) */
    int64_t ld_y;
    double* Out;        /* rows x f at pitch ld_out; must not alias an input */
    int64_t ld_out;
    int f;              /* head width */
    int softmax;        /* column pass: P carries lse and delta (row pass: implied by lse != NULL) */
    double leaky_alpha;
} hnh_attn_grad;

/* Row pass over a block of S (or a window of it):  Out_i (+)= sum_j de_ij Y_j.
 * Column pass over a block of S^T:                 Out_j (+)= sum_i a_ij P_i[fp : fp + f] + de_ij P_i[0 : f].
 * flags: HNH_FUSED_OUT_OVERWRITE or 0.  b->rowptr == NULL: a block of b->rows rows without any nonzero (HNH_FUSED_OUT_OVERWRITE
 * stores zeros, otherwise nothing happens).  Windows, structure plans and the Infinity-Cache panels as for hnh_fused_sddmm_spmm_csr_p. */
int hnh_attn_grad_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* window,
                            int stream);
int hnh_attn_grad_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* window,
                            int stream);

/* P[r, :] = [A[r, 0 : f] (0) | dZ[r, 0 : f] (0) | lse[r] delta[r]] for r < rows, in the layout above; lse == delta == NULL: attention
 * none (no scalars).  ld_p must be even and at least the packed width; columns of P beyond the packed width are not touched. */
int hnh_attn_grad_pack_f64(hnh_ctx* ctx, double* P, int64_t ld_p, const double* A, int64_t ld_a, const double* dZ, int64_t ld_dz,
                           const double* lse, const double* delta, int64_t rows, int f, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_GRAD_H */
