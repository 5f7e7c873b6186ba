/*
 * hnh_attn_edge.h — a per-edge bias on the logits of the query/key/value attention (GAT score "transformer" with GAT::set_edge_bias,
 * csrc/host/gat.hpp), forward and backward, exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_attn_qkv.h, whose three passes these are with one more operand: the host layer
 * binds it with dlsym and leaves it null when a kernel library does not export it (neither CPU test double under oracle/ does); a GAT layer
 * with an edge bias then fails with an error naming the missing symbol, and nothing else needs it.
 *
 * bias holds one FINITE fp64 value per nonzero of the block, b_e for entry e of the block's CSR order.  It belongs to the entry, not to the
 * pair (i, j): two copies of a repeated pair may carry different values.  With the definitions of hnh_attn_qkv.h,
 *     s_e = scale <Q_i, K_j> + b_e     lse_i = log sum_e exp(s_e)     p_e = exp(s_e - lse_i)     o_i = sum_e p_e V_j                (forward)
 *     delta_i, g_e = scale p_e (<dZ_i, V_j> - delta_i), dQ, dK, dV as there, with p_e from the biased s_e                          (backward)
 * so b_e = log w_e gives the weighted neighbourhood softmax p_e ~ w_e exp(scale <Q_i, K_j>).  The entry points of this header treat the
 * bias as a constant; dL/db_e = g_e / scale is returned by the backward passes' twins of include/hnh_attn_edge_grad.h, a group of its own.
 *
 * Addressing: bias is addressed exactly as hnh_sddmm_csr_ps addresses `values`: bias[e], e in the BLOCK's numbering, whatever window,
 * group of windows, Infinity-Cache panel or hub-row segment the nonzero is visited in; it may be a slice of a caller's longer vector.  The
 * column pass's block is a block of S^T and its bias is in S^T's order: the caller keeps the two orders in agreement.  The forward pass's
 * optional values[e] receives the BIASED logit.
 *
 * Values: finite.  A very negative value, such as -1e300, removes an edge from every row that keeps another edge of moderate bias: its p_e
 * underflows to an exact 0, forward and backward.  -inf is NOT supported: the online softmax's empty state is a running maximum of -inf,
 * and an edge at -inf would meet (-inf) - (-inf).  +inf and NaN are not supported either.
 *
 * Magnitudes.  The backward passes recompute p_e = exp((scale <Q_i, K_j> - lse_i) + b_e) from the stored lse_i, which is about as large as
 * the row's largest bias, so the exponent carries an absolute error of up to ulp(lse_i): rows whose largest bias lies within +-1e6 keep
 * p_e to 1e-10, and beyond that the gradients of the row lose digits in proportion.  The extreme: a row whose edges are ALL at -1e300.  With
 * ONE edge it is exact (lse_i = -1e300 absorbs the score, p_e = exp(0) = 1 in every pass, like any single edge).  With SEVERAL edges it is NOT
 * supported: the forward pass gives the uniform 1 / degree, but lse_i = -1e300 has absorbed log(degree), and the backward passes see
 * p_e = 1: dV is wrong by the factor degree.  Nothing here looks for such rows (GAT.edge_bias_from of the Python layer refuses them).
 *
 * Everything else is the parents' contract to the letter: struct hnh_attn_qkv (unchanged, 168 bytes), the flags, the row-state protocol,
 * HNH_ATTN_FINISH and HNH_ATTN_ADDEND, the activations, b->rowptr == NULL, HNH_ATTN_QKV_MAX_F with HNH_ERR_UNSUPPORTED, no atomics, hub
 * rows whole in the forward pass and in 256-nonzero segments in the backward passes; results are bit-identical run to run and for any
 * split into windows, panels or groups of windows, and with an all-zero bias bit-identical to the parents'.  bias == NULL on a block with
 * nonzeros (b->rowptr != NULL) is an error (HNH_ERR_INVALID, nothing written), never a fall-back to the parent, checked behind the parents'
 * own refusals of flags and head width (a head beyond the limit is HNH_ERR_UNSUPPORTED with or without a bias); a block without nonzeros
 * has no entry to address and its bias is not looked at.
 */
#ifndef HNH_ATTN_EDGE_H
#define HNH_ATTN_EDGE_H
#include "hnh_attn_qkv.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hnh_attn_qkv_fwd_csr_p with s_e = scale <Q_i, K_j> + bias[e] */
int hnh_attn_qkv_bias_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream);

/* hnh_attn_qkv_row_csr_p (a block of S, bias in S's order) and hnh_attn_qkv_col_csr_p (a block of S^T, bias in S^T's order: nonzero
 * (j, i) of the block carries the bias of S_ij) with p_e from the biased logit */
int hnh_attn_qkv_bias_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream);
int hnh_attn_qkv_bias_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_EDGE_H */
