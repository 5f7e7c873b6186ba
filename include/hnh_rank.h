/*
 * hnh_rank.h — exact item ranks for implicit-feedback ALS (Implicit_ALS::rank_of in csrc/host/als_implicit.hpp): for a batch of query
 * rows and a few targets per row, HOW MANY items rank before each target in the total order of include/hnh_topk.h, counted while the score
 * tile is still in the accumulators of the fp64 matrix cores: neither the nq x n score matrix nor a tile of it is written anywhere.  The
 * sibling of hnh_topk_rows_f64 with a cheaper epilogue, the scores of single pairs, and the subtraction of excluded items.  Exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_topk.h: the host layer binds it with dlsym and leaves it null when a kernel library
 * does not export it (neither CPU test double under oracle/ does); Implicit_ALS::rank_of then fails with an error naming the missing
 * symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers (ONE exception, marked HOST below), row-major fp64,
 * int status, asynchronous on the given stream.  No atomics on global memory.
 *
 * THE TOTAL ORDER is that of include/hnh_topk.h: candidate (s, id) ranks before (s', id') when s > s', or when s == s' and id < id'.
 * Scores compare as numbers (-0.0 equals +0.0).  Operands and target scores must be finite: behaviour on NaN is NOT defined.
 *
 * THREE PROPERTIES.
 *   1. hnh_pair_scores_f64 returns for a pair THE VERY BITS that hnh_topk_rows_f64 returns in out_scores for it, and that the counting
 *      pass compares: the products are accumulated in ascending k by v_mfma_f64_16x16x4_f64, four k's a step, in all three kernels; a
 *      score's bits depend on its two rows and R only.
 *   2. A count is an exact int64: the number of items j < n whose (<Q_q, Y_j>, id_base + j) ranks before the target.  An item never ranks
 *      before itself, so a target that is item j of Y with the score of property 1 gets its 0-based position in the query's full ordering.
 *   3. A count is additive over any partition of the items, so it is the same integer for any `splits`, for any partition of Y over
 *      calls whose counts are added, and for any position of the query in its batch.
 */
#ifndef HNH_RANK_H
#define HNH_RANK_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_RANK_MAX_R 512      /* the widest row */
#define HNH_RANK_MAX_TARGETS 16 /* the most targets of one query row */
#define HNH_RANK_MAX_SPLITS 1024 /* the most item ranges of one call */

/* out[p] = <Q[pair_q[p]], Y[pair_j[p]]> for p < npairs (Q is nq x R, Y is n x R; pair_q and pair_j are int64), with the bits of property
 * 1.  A pair_q outside [0, nq) or a pair_j outside [0, n) gives +0.0, so that a sum of such arrays over the holders of the items is
 * exact.  1 <= R <= HNH_RANK_MAX_R; npairs == 0: nothing is launched.  16-byte loads are used only where base and pitch allow. */
int hnh_pair_scores_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, const int64_t* pair_q, const int64_t* pair_j,
                        int64_t npairs, double* out, int stream);

/* Bytes of `work` that hnh_rank_rows_f64 needs for nq query rows, n items, ntargets targets in all and `splits` (0: the library's choice,
 * as in the call); -1 for arguments that the call would refuse. */
int64_t hnh_rank_rows_f64_workspace(int64_t nq, int64_t n, int64_t ntargets, int splits);

/* For every query row q < nq of Q (nq x R) and every target t in tgt_ptr[q] .. tgt_ptr[q + 1]:
 *     counts[t] = #{ j < n : (<Q_q, Y_j>, id_base + j) ranks before (tgt_score[t], tgt_id[t]) }          (int64, property 2)
 *   tgt_ptr: HOST array of nq + 1 ascending offsets from 0 (it is checked before anything is launched, and the call keeps a copy in
 *   `work`: the array may go when the call returns).  A row has at most HNH_RANK_MAX_TARGETS targets: a user with more is given several
 *   query rows.  tgt_score, tgt_id, counts: device arrays of tgt_ptr[nq] entries; a target need not be an item of Y, and a target may
 *   be repeated.
 *   splits: the number of item ranges that are counted independently into `work` and then summed by a second small launch; 0 lets the
 *   library choose, 1 .. HNH_RANK_MAX_SPLITS forces it.  The result does not depend on it (property 3).
 *   work, work_bytes: scratch of at least hnh_rank_rows_f64_workspace() bytes, 16-byte aligned; its contents are undefined afterwards.
 * 1 <= R <= HNH_RANK_MAX_R, any nq >= 0 and n >= 0 (nq == 0 or no target: nothing is launched; n == 0: every count is 0),
 * 0 <= id_base <= INT64_MAX - n; remainders in nq, n and R are handled, and 16-byte loads are used only where base and pitch allow.  Q, Y
 * and the targets are read only.  Anything else fails with HNH_ERR_INVALID and a message, and nothing is launched or written. */
int hnh_rank_rows_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, int64_t id_base, const int64_t* tgt_ptr,
                      const double* tgt_score, const int64_t* tgt_id, int splits, int64_t* counts, void* work, int64_t work_bytes, int stream);

/* counts[t] -= #{ e in excl_ptr[q] .. excl_ptr[q + 1] : (excl_score[e], excl_id[e]) ranks before (tgt_score[t], tgt_id[t]) } for every
 * query q < nq and every target t in tgt_ptr[q] .. tgt_ptr[q + 1].  Here tgt_ptr and excl_ptr are DEVICE arrays of nq + 1 int64 offsets;
 * any number of targets and of entries per query.  With excl_score from hnh_pair_scores_f64 the entries carry the bits that the counting
 * pass compared (property 1), so the difference is the exact count over the items that are not excluded; an entry that is the target
 * itself does not rank before it.  One wave per query: not a hot path. */
int hnh_rank_exclude_f64(hnh_ctx* ctx, int64_t nq, const int64_t* excl_ptr, const double* excl_score, const int64_t* excl_id, const int64_t* tgt_ptr,
                         const double* tgt_score, const int64_t* tgt_id, int64_t* counts, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_RANK_H */
