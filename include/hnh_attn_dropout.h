/*
 * hnh_attn_dropout.h — dropout for the GAT (csrc/host/gat.hpp, GAT::set_dropout): on the normalised attention coefficients of the additive
 * score (include/hnh_attn_additive.h) and on a layer's input, with masks RECOMPUTED from a stateless counter-based generator.  Exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h, include/hnh_attention.h, include/hnh_attn_grad.h and
 * include/hnh_attn_additive.h: the host layer binds it with dlsym and leaves it null when a kernel library does not export it (neither CPU test double under oracle/ does); dropout then fails with an error naming the missing symbol, and nothing else needs it.
 *
 * The mask.  Philox-4x32 with 10 rounds (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85):
 *     key     = (seed & 0xffffffff, seed >> 32)                      for a 64-bit seed
 *     counter = (gi, gj, w2, stream_tag)
 *     attention mask of edge (i, j), head h of layer l:   gi = global row, gj = global column, w2 = l * 65536 + h, stream_tag = 0
 *     feature mask of entry (r, k) of layer l's input:    gi = r,          gj = k,             w2 = l,             stream_tag = 1
 *     kept iff output word 0 >= threshold,  threshold = floor(p * 2^32) as a uint32 computed on the host
 *     kept values are scaled by scale = 1 / (1 - p), an fp64 value computed on the host
 * The keep test is an integer comparison: the mask is bit-exact on every device and on the host (hnh_dropout_word, include/hnh_dist.h).
 * Global ids are the operator's own numbering.  Nothing is stored per nonzero: the forward pass over S, the backward row pass over S and
 * the backward column pass over S^T (on other ranks, through other windows, panels and hub-row segments) each recompute the same word
 * from the same key.  A repeated pair (i, j) has the same key, so EVERY COPY of a repeated edge gets the same mask.
 *
 * Mathematics, with m_ij in {0, 1}, c = scale, everything else as in hnh_attn_additive.h:
 *     lse_i, a_ij unchanged (the normalisation runs over ALL edges)          o_i = sum_j c m_ij a_ij A_j
 *     (online softmax: l takes every edge, acc the kept ones times c; a row whose edges are all dropped gives o_i = 0 and keeps lse_i)
 *     delta_i = <dZ_i, o_i>     dz_ij = a_ij (c m_ij <dZ_i, A_j> - delta_i) g(z_ij)     dAgg_j = sum_i c m_ij a_ij dZ_i
 *     ds, dt and the rank-2 update as in hnh_attn_additive.h
 *
 * The gathered row's global id TRAVELS IN THE OPERAND, as its scalars do, stored as a double (exact below 2^53; checked to fit 32 bits by
 * the caller); a schedule's relabelling of columns to landing-buffer rows never matters.  fp = f rounded up to even:
 *
 *     scored operand   M'_r = [ A_r[0 : f] (pad) | s_r t_r | id_r 0 ]           HNH_ATTN_DROP_SCORED_WIDTH(f) = fp + 4 doubles
 *     packed operand   Q'_r = [ dZ_r[0 : f] (pad) | s_r lse_r delta_r id_r ]    HNH_ATTN_ADD_PACKED_WIDTH(f)  = fp + 4 doubles (unchanged)
 *
 * The own row's id is row_id0 plus the local row.  The forward and the row pass take one more 16-byte load per gathered row than their
 * parents, the column pass none (it loads the slot already).
 */
#ifndef HNH_ATTN_DROPOUT_H
#define HNH_ATTN_DROPOUT_H
#include "hnh_attn_additive.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_DROP_SCORED_WIDTH(f) ((f) + ((f) & 1) + 4)
#define HNH_DROPOUT_STREAM_ATTENTION 0u
#define HNH_DROPOUT_STREAM_FEATURE 1u

typedef struct hnh_attn_drop {
    uint64_t seed;
    uint32_t w2;        /* layer * 65536 + head */
    uint32_t threshold; /* floor(p * 2^32) */
    double scale;       /* 1 / (1 - p) */
    int64_t row_id0;    /* global id of the block's row 0 (a row of S for the forward and the row pass, a column of S for the column pass) */
} hnh_attn_drop;

/* The three passes of hnh_attn_additive.h with the mask: same arguments, flags, windows, plans, panels, hub-row segments and row-state
 * protocol as hnh_attn_add_fwd_csr_p / _row_csr_p / _col_csr_p.  args->Y is M' (forward, row pass; pitch >= fp + 4) or Q' (column pass);
 * args->M is the block's own rows of M' (or of M: only columns below fp + 2 are read).  The block's row ids must fit 32 bits. */
int hnh_attn_drop_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream);
int hnh_attn_drop_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream);
int hnh_attn_drop_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream);

/* M'[r, :] = [A[r, 0 : f] (0) | <A_r, a1> <A_r, a2> | row_id0 + r, 0] for r < rows.  ld_m even and >= fp + 4; M' must not alias A. */
int hnh_attn_drop_scores_f64(hnh_ctx* ctx, double* M, int64_t ld_m, const double* A, int64_t ld_a, const double* a1, const double* a2,
                             int64_t rows, int f, int64_t row_id0, int stream);

/* Q'[r, :] = [dZ[r, 0 : f] (0) | M[r, fp] lse[r] delta[r] row_id0 + r] for r < rows.  ld_q even and >= fp + 4. */
int hnh_attn_drop_pack_f64(hnh_ctx* ctx, double* Q, int64_t ld_q, const double* dZ, int64_t ld_dz, const double* M, int64_t ld_m,
                           const double* lse, const double* delta, int64_t rows, int f, int64_t row_id0, int stream);

/* dst[r, k] = scale * mask(row_id0 + r, k) * src[r, k] for r < rows, k < cols, the feature mask above (stream_tag 1, w2 = the layer).
 * dst == src is allowed.  Serves the forward copy Xd = c mask o X and the gradient c mask o dX alike. */
int hnh_feat_drop_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, const double* src, int64_t ld_src, int64_t rows, int64_t cols,
                      int64_t row_id0, uint64_t seed, uint32_t w2, uint32_t threshold, double scale, int stream);

/* out[k] = word 0 of Philox(counter = (gi[k], gj[k], w2, stream_tag), key = seed) for k < n: the device generator on its own. */
int hnh_dropout_words_u32(hnh_ctx* ctx, uint32_t* out, const uint32_t* gi, const uint32_t* gj, int64_t n, uint64_t seed, uint32_t w2,
                          uint32_t stream_tag, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_DROPOUT_H */
