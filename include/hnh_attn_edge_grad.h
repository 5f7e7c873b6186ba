/*
 * hnh_attn_edge_grad.h — the gradient of the per-edge bias of include/hnh_attn_edge.h: the two biased backward passes of the
 * query/key/value attention with one more result, dL/db_e per nonzero (GAT::set_edge_bias_learned, csrc/host/gat.hpp), exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_attn_edge.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); a GAT layer whose edge bias is learned then fails with an error
 * naming the missing symbol, and nothing else needs it.
 *
 * With the definitions of hnh_attn_qkv.h and hnh_attn_edge.h, for ONE head
 *     dL/db_e = p_e (<dZ_i, V_j> - delta_i)        (= g_e / scale)
 * which both backward passes hold for every nonzero after their butterfly reduction (the row pass for entry e = (i, j) of S, the column
 * pass for the same nonzero as entry (j, i) of S^T, from the gathered row's lse_i and delta_i): nothing more is gathered.  The caller adds
 * the heads of a layer that share a bias by passing accumulate = 0 for the first head and accumulate != 0 for the others; the sum is then
 * formed in the order of the calls.  An entry whose p_e underflows to 0 (a switched-off edge at -1e300 next to an edge of moderate bias)
 * gets an exact 0.0, and so does the single edge of a row at any bias where <dZ_i, V_j> equals delta_i (p_e = 1).
 *
 * dbias is addressed exactly as bias is: dbias[e], e in the BLOCK's numbering, whatever window, group of windows, Infinity-Cache panel or
 * 256-nonzero hub-row segment the nonzero is visited in; it may be a slice of a caller's longer vector.  Every nonzero is visited by
 * exactly one (launch, segment), whose owning lane stores 8 bytes (accumulate: loads, adds, stores): no partial rows, no atomics, and
 * results that are bit-identical run to run and for any split into windows, panels or groups of windows.  The row pass writes S's order,
 * the column pass S^T's.  A call over a window writes the entries of that window's nonzeros and no others.
 *
 * Everything else is hnh_attn_qkv_bias_row_csr_p / hnh_attn_qkv_bias_col_csr_p to the letter: the same Out / Out2 bit for bit, the same
 * refusals in the same order, struct hnh_attn_qkv unchanged (168 bytes).  `accumulate` is an argument of its own, not a bit of `flags`, and
 * independent of HNH_FUSED_OUT_OVERWRITE, which keeps governing Out and Out2.  dbias == NULL on a block with nonzeros
 * (b->rowptr != NULL) is an error (HNH_ERR_INVALID, nothing written), checked behind the parents' refusals and the null bias; a block
 * with b->rowptr == NULL touches no dbias.  dbias must not overlap bias or any other operand.
 */
#ifndef HNH_ATTN_EDGE_GRAD_H
#define HNH_ATTN_EDGE_GRAD_H
#include "hnh_attn_edge.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hnh_attn_qkv_bias_row_csr_p (a block of S; bias and dbias in S's order) with dbias[e] (+)= p_e (<dZ_i, V_j> - delta_i) */
int hnh_attn_qkv_bias_grad_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, double* dbias,
                                     int accumulate, unsigned flags, const hnh_csr_window* window, int stream);
/* hnh_attn_qkv_bias_col_csr_p (a block of S^T; bias and dbias in S^T's order: nonzero (j, i) of the block is S_ij) with the same result */
int hnh_attn_qkv_bias_grad_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, double* dbias,
                                     int accumulate, unsigned flags, const hnh_csr_window* window, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_EDGE_GRAD_H */
