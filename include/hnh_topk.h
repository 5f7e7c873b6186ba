/*
 * hnh_topk.h — the serving side of implicit-feedback ALS (Implicit_ALS::recommend in csrc/host/als_implicit.hpp): for a batch of query
 * rows, the k items with the largest inner products, selected while the score tile is still in the accumulators of the fp64 matrix
 * cores, so that the nq x n score matrix is never written; the merge of several such lists, and a row gather.  Exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_als_implicit.h: the host layer binds it with dlsym and leaves it null when a
 * kernel library does not export it (neither CPU test double under oracle/ does); Implicit_ALS::recommend then fails with an error naming
 * the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status,
 * asynchronous on the given stream.  No atomics on global memory.
 *
 * THE TOTAL ORDER.  Candidate (s, id) ranks before (s', id') when s > s', or when s == s' and id < id'.  Scores compare as numbers
 * (-0.0 equals +0.0).  Operands must be finite: behaviour on NaN is NOT defined.  Ids of one call are distinct, so the order is strict
 * and the first k of a set do not depend on the order in which the set is searched or merged.
 *
 * A SCORE'S BITS depend only on the two rows and on R: the products are accumulated in ascending k by v_mfma_f64_16x16x4_f64, four k's a
 * step, whatever nq, n, the rows' positions in their tiles, `splits`, or the rank that holds the item.  Kernel instances are chosen by R
 * alone.  With the total order, the whole result is therefore bit-identical for any `splits` and any partition of the items over calls
 * whose lists are merged with hnh_topk_merge_f64.
 */
#ifndef HNH_TOPK_H
#define HNH_TOPK_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_TOPK_MAX_K 128       /* the longest list */
#define HNH_TOPK_MAX_R 512       /* the widest row */
#define HNH_TOPK_MAX_SPLITS 1024 /* the most item ranges of one call */

/* Bytes of `work` that hnh_topk_rows_f64 needs with splits = 0, or with any forced 1 <= splits <= 8 (a larger forced count needs more,
 * and the call then says how much); -1 for arguments that the call would refuse. */
int64_t hnh_topk_rows_f64_workspace(int64_t nq, int64_t n, int R, int k);

/* For every query row q < nq of Q (nq x R), the first k items j < n of Y (n x R) in the total order of (<Q_q, Y_j>, id_base + j), skipping
 * every j in excl_idx[excl_ptr[q] .. excl_ptr[q + 1]) (local row numbers of Y, ascending and without repeats; excl_ptr == NULL: nothing
 * is excluded).  An excluded item is never returned and never displaces another, whatever its score.
 *   out_scores, out_ids: nq x k, best first; out_ids holds id_base + j.  Where fewer than k items are left the tail is id -1 with score
 *   -infinity.
 *   splits: the number of item ranges that are searched independently and then merged (by the kernel of hnh_topk_merge_f64); 0 lets the
 *   library choose, 1 .. HNH_TOPK_MAX_SPLITS forces it.  The result does not depend on it.
 *   work, work_bytes: scratch of at least hnh_topk_rows_f64_workspace() bytes, 16-byte aligned; its contents are undefined afterwards.
 * 1 <= k <= HNH_TOPK_MAX_K, 1 <= R <= HNH_TOPK_MAX_R, any nq >= 0 and n >= 0 (nq == 0: nothing is launched; n == 0: every entry is
 * empty), 0 <= id_base <= INT64_MAX - n (a negative id would read as an empty entry in a merged list); remainders in nq, n and R are handled, and 16-byte loads are used only where base and pitch allow.  Q, Y and the lists are
 * read only.  Anything else fails with HNH_ERR_INVALID and a message, and nothing is launched. */
int hnh_topk_rows_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, int64_t id_base, const int64_t* excl_ptr,
                      const int32_t* excl_idx, int k, int splits, double* out_scores, int64_t* out_ids, void* work, int64_t work_bytes, int stream);

/* The first k of the union of `parts` lists per query in the total order: in_scores and in_ids are laid out [part][nq][k], real ids are
 * >= 0 and EVERY negative id is an empty entry (the lists of hnh_topk_rows_f64 use -1; the score of an empty entry is ignored, NaN
 * included), all real ids of a query are distinct.  A score keeps its bits (the sign of a zero too).  out_scores, out_ids: nq x k, best
 * first, the tail (-infinity, -1).  The outputs must not overlap the inputs.  parts >= 1, nq >= 0, 1 <= k <= HNH_TOPK_MAX_K. */
int hnh_topk_merge_f64(hnh_ctx* ctx, const double* in_scores, const int64_t* in_ids, int parts, int64_t nq, int k, double* out_scores,
                       int64_t* out_ids, int stream);

/* out[q, :] = X[idx[q], :] for q < nq where 0 <= idx[q] < rows, and a row of +0.0 otherwise (X is rows x R, out nq x R). */
int hnh_take_rows_f64(hnh_ctx* ctx, const double* X, int64_t rows, int R, const int64_t* idx, int64_t nq, double* out, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_TOPK_H */
