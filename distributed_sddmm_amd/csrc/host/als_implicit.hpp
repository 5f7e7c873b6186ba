// Implicit-feedback ALS with confidence weights (Hu, Koren and Volinsky), every row solved by a few CG iterations (Takacs' method): an
// addition beside Distributed_ALS, which stays the reference's benchmark.  No counterpart in the reference.
//
// The model.  S has a stored pair per observed (i, j) and a weight w_e >= 0 on it: confidence c_e = 1 + w_e, preference 1 on the stored
// pairs and 0 on every other of the M N pairs (confidence 1 there), lambda > 0:
//     L(A, B) = sum over ALL i, j of c_ij (p_ij - <a_i, b_j>)^2 + lambda (|A|^2 + |B|^2)
//             = sum_{e in S} [(1 + w_e)(1 - s_e)^2 - s_e^2] + <A^T A, B^T B>_F + lambda (|A|_F^2 + |B|_F^2),     s_e = <a_i, b_j>.
// Half-step for X with Y fixed, G = Y^T Y (R x R, summed over all ranks): row i solves (G + Y_i^T diag(w) Y_i + lambda I) x_i = rhs_i,
//     rhs_i = sum_{e in row i} (1 + w_e) y_j          M(x)_i = sum_e w_e <x_i, y_j> y_j + lambda x_i + x_i G
// by CG from the current x_i:  r = rhs - M(x), p = r, rs_i = <r_i, r_i>, then `iters` times per row
//     Mp = M(p)_i;  bdot = <p_i, Mp>;  live = rs_i > 0 and bdot > 0;  alpha = live ? rs_i / bdot : 0;  x_i += alpha p_i;  r_i -= alpha Mp;
//     rsnew = <r_i, r_i>;  beta = live ? rsnew / rs_i : 0;  p_i = r_i + beta p_i;  rs_i = rsnew.
// There is no epsilon (ALS_CG::cg_optimizer's nan_avoidance_constant, added to both rsold and <p, Mp>, makes alpha tend to 1 on a row
// that has converged, and the iterate runs away: harmless in the benchmark, whose systems never converge, fatal here): a row that is not
// live keeps x_i and r_i.  Empty rows and the padding rows of a rank's block are ordinary rows (M = G + lambda I, rhs = 0).
//
// An iteration is ONE weighted fused SDDMM -> SpMM call (Sparse15D_Dense_Shift::fusedSpMM_out with the weights w, x_scale = lambda) plus
// the Gram term and the row updates:
//   folded    hnh_gram_rows_f64 (include/hnh_als_implicit.h, an optional kernel group) adds p G on the matrix cores and runs the guarded
//             update on the row while it is on chip: 7 matrix passes.  R <= HNH_GRAM_MAX_R.
//   composed  hnh_gemm_f64 (p G), hnh_axpy_f64, hnh_rowdot_f64, the guarded scalars, hnh_cg_step_f64 and hnh_row_scale_add_f64.  The
//             guarded scalars need a select, which hnh_relu_grad_cols_f64 (include/hnh_grad.h: dZ = out > 0 ? G : 0) on a one-column
//             matrix is: alpha = bdot > 0 ? rs / bdot : 0 (rs == 0 gives 0 by itself) and beta = bdot > 0 ? (rs > 0 ? rsnew / rs : 0) : 0.
//             No helper was added for it.  Any R; the only mode for R > HNH_GRAM_MAX_R.
// Both need hnh_gemm_tn_f64 of include/hnh_grad.h for the Gram matrices; a kernel library without a needed group is refused through
// Backend::missing_kernel().  Schedule: 15d_fusion2 only (c = 1 and c > 1): its fused pass takes the weights, and its layout gives every
// rank distinct rows of A and of B, so the Gram matrix is the sum of the ranks' own.
//
// Serving.  recommend() returns, for a batch of users, the k items with the largest <a_u, b_j> in the total order of include/hnh_topk.h
// (score descending, then item id ascending), with or without the items of the user's row of S.  Every rank searches its own valid rows
// of B with hnh_topk_rows_f64 (scores and selection in one kernel: no M x N product is stored anywhere), the ranks' lists are all-gathered
// and merged by hnh_topk_merge_f64.  A score's bits depend on its two rows and R only, and the order is strict, so every rank count gives
// the same bits.  The exclusion lists come from the GLOBAL coordinates of the rank's stored pairs, which the schedule does not keep: they
// are read back once, by two SDDMM calls on probe matrices (row ids against ones, ones against column ids), and cached in the object.
//
// Evaluation.  rank_of() returns the exact position of an item in a user's full ordering of all N items (the order of recommend) by
// COUNTING on the device (include/hnh_rank.h: the top-k kernel's product loop with a counting epilogue, no score stored); the counts are
// integers and additive over the ranks' rows of B, so every rank count gives the same numbers.  AUC, MPR and MRR are host arithmetic on them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include "dense_shift_15d.hpp"

class Implicit_ALS {
public:
    Sparse15D_Dense_Shift* d_ops = nullptr;
    DenseMatrix A, B;
    double lambda;
    uint64_t seed;

    Implicit_ALS(Distributed_Sparse* ops, double lambda_in, uint64_t seed_in = 2022) : lambda(lambda_in), seed(seed_in) {
        d_ops = dynamic_cast<Sparse15D_Dense_Shift*>(ops);
        if (d_ops == nullptr || d_ops->fusionApproach != 2)
            throw hnh::Error("Error, Implicit_ALS supports the schedule 15d_fusion2 only, not " +
                             (d_ops ? "15d_fusion" + std::to_string(d_ops->fusionApproach) + " (" + ops->algorithm_name + ")" : ops->algorithm_name));
        if (!(lambda > 0.0) || !std::isfinite(lambda)) throw hnh::Error("Error, Implicit_ALS needs a finite lambda > 0!");
        folded_ = d_ops->world->be->hnh_gram_rows_f64 != nullptr;  // (the measured default: see set_folded)
    }
    ~Implicit_ALS() {
        if (d_ops) d_ops->forget_fused_weights();
    }

    // w >= 0 per stored pair in the like_S_values and the like_ST_values layouts (the same weights, keyed both ways).  Kept as w and 1 + w.
    void set_confidence(const VectorXd& w_S, const VectorXd& w_ST) {
        VectorXd ls = d_ops->like_S_values(1.0), lst = d_ops->like_ST_values(1.0);
        if (w_S.size() != ls.size() || w_ST.size() != lst.size()) throw hnh::Error("Error, Implicit_ALS set_confidence: the weight vectors have the wrong length!");
        std::vector<double> hs = w_S.to_host(), hst = w_ST.to_host();
        for (const std::vector<double>* h : {&hs, &hst})
            for (double v : *h)
                if (!(v >= 0.0) || !std::isfinite(v)) throw hnh::Error("Error, Implicit_ALS set_confidence needs finite weights >= 0!");
        hnh::World* w = d_ops->world;
        d_ops->forget_fused_weights();
        w_S_ = VectorXd(ls.size());
        w_ST_ = VectorXd(lst.size());
        w->copy(w_S_.data(), w_S.data(), (size_t)ls.size() * sizeof(double), HNH_COPY_D2D, HNH_STREAM_COMPUTE);
        w->copy(w_ST_.data(), w_ST.data(), (size_t)lst.size() * sizeof(double), HNH_COPY_D2D, HNH_STREAM_COMPUTE);
        if (ls.size()) w->check(w->be->hnh_axpy_f64(w->ctx, ls.data(), w_S_.data(), 1.0, ls.size(), HNH_STREAM_COMPUTE), "hnh_axpy_f64");
        if (lst.size()) w->check(w->be->hnh_axpy_f64(w->ctx, lst.data(), w_ST_.data(), 1.0, lst.size(), HNH_STREAM_COMPUTE), "hnh_axpy_f64");
        c_S_ = std::move(ls);
        c_ST_ = std::move(lst);
        w_host_ = std::move(hs);
        confidence_set_ = true;
    }

    void initializeEmbeddings() {  // Distributed_ALS's hashed fill: the same factors for every rank count
        A = d_ops->like_A_matrix(0.0);
        B = d_ops->like_B_matrix(0.0);
        hashed_fill(A, Amat, seed + 3, 1.4 / (double)d_ops->R);
        hashed_fill(B, Bmat, seed + 4, 1.0 / (1.3 * (double)d_ops->R));
    }
    void set_embeddings(const DenseMatrix& a, const DenseMatrix& b) {
        if (a.rows() != d_ops->localArows || a.cols() != d_ops->R || b.rows() != d_ops->localBrows || b.cols() != d_ops->R)
            throw hnh::Error("Error, Implicit_ALS set_embeddings: the factors have the wrong shape!");
        A = a;
        B = b;
    }

    // true: hnh_gram_rows_f64 runs the Gram term and the guarded update in one launch; false: the composed sequence.  The default is
    // folded where the kernel library has the group: it measured faster.
    void set_folded(bool on) { folded_ = on; }
    bool folded() const { return folded_; }

    // G = X^T X over the valid rows of every rank, all-reduced; `host` receives R * R doubles
    void gram(MatMode which, double* host) {
        require_embeddings("gram");
        DenseMatrix G = gram_of(which == Amat ? A : B, which);
        G.copy_to_host(host);
    }

    void half_step(MatMode matrix_to_optimize, int iters) {
        require_embeddings("half_step");
        if (!confidence_set_) throw hnh::Error("Error, Implicit_ALS half_step needs set_confidence first!");
        if (iters < 0) throw hnh::Error("Error, Implicit_ALS half_step needs iters >= 0!");
        hnh::World* w = d_ops->world;
        hnh::Backend* be = w->be;
        const int R = (int)d_ops->R;
        if (folded_) {
            if (be->hnh_gram_rows_f64 == nullptr) throw hnh::Error(be->missing_kernel("Implicit_ALS in folded mode", "hnh_gram_rows_f64"));
            if (R > HNH_GRAM_MAX_R)
                throw hnh::Error("Error, Implicit_ALS in folded mode supports R <= " + std::to_string(HNH_GRAM_MAX_R) + ", not R = " + std::to_string(R) +
                                 ": use set_folded(false)");
        } else if (be->hnh_relu_grad_cols_f64 == nullptr) {
            throw hnh::Error(be->missing_kernel("Implicit_ALS in composed mode", "hnh_relu_grad_cols_f64"));
        }
        const bool a_side = matrix_to_optimize == Amat;
        DenseMatrix& X = a_side ? A : B;
        DenseMatrix& Y = a_side ? B : A;
        const VectorXd& wv = a_side ? w_S_ : w_ST_;
        const int64_t nrows = X.rows();
        const int64_t n = nrows * R;

        struct Hold {
            Distributed_Sparse* d;
            Hold(Distributed_Sparse* d_in, const DenseMatrix* m) : d(d_in) { d->hold_moving_operand(m); }
            ~Hold() { d->release_moving_operand(); }
        } hold(d_ops, &Y);

        DenseMatrix G = gram_of(Y, a_side ? Bmat : Amat);
        DenseMatrix r(nrows, R), Mp(nrows, R), T;
        r.setZero();
        if (a_side) d_ops->spmmA(r, Y, c_S_);  // rhs = sum (1 + w) y
        else d_ops->spmmB(Y, r, c_ST_);

        // Mp = M(x): the weighted fused call with + lambda x, then + x G
        auto apply = [&](DenseMatrix& x, const hnh_gram_cg* cg) {
            const hnh_fused_extras ex = {0.0, lambda, nullptr, nullptr, nullptr, 0};
            if (a_side) d_ops->fusedSpMM_out(x, Y, Amat, Mp, ex, wv);
            else d_ops->fusedSpMM_out(Y, x, Bmat, Mp, ex, wv);
            if (folded_) {
                w->check(be->hnh_gram_rows_f64(w->ctx, Mp.data(), x.data(), G.data(), nrows, R, nullptr, cg, HNH_STREAM_COMPUTE), "hnh_gram_rows_f64");
            } else {
                if (T.rows() != nrows) T = DenseMatrix(nrows, R);
                w->check(be->hnh_gemm_f64(w->ctx, nrows, R, R, x.data(), G.data(), T.data(), HNH_STREAM_COMPUTE), "hnh_gemm_f64");
                w->check(be->hnh_axpy_f64(w->ctx, Mp.data(), T.data(), 1.0, n, HNH_STREAM_COMPUTE), "hnh_axpy_f64");
            }
        };
        apply(X, nullptr);
        w->check(be->hnh_row_scale_add_f64(w->ctx, r.data(), nullptr, 1.0, Mp.data(), nullptr, -1.0, nrows, R, HNH_STREAM_COMPUTE), "hnh_row_scale_add_f64");
        DenseMatrix p = r;
        VectorXd rs(nrows), rsnew, bdot, quot, alpha, beta;
        w->check(be->hnh_rowdot_f64(w->ctx, r.data(), r.data(), rs.data(), nrows, R, HNH_STREAM_COMPUTE), "hnh_rowdot_f64");
        if (!folded_) {
            rsnew = VectorXd(nrows); bdot = VectorXd(nrows); quot = VectorXd(nrows); alpha = VectorXd(nrows); beta = VectorXd(nrows);
        }
        // out[i] = cond[i] > 0 ? value[i] : 0
        auto select = [&](VectorXd& out, const VectorXd& value, const VectorXd& cond) {
            w->check(be->hnh_relu_grad_cols_f64(w->ctx, out.data(), 1, value.data(), 1, cond.data(), 1, 0, nrows, 1, HNH_STREAM_COMPUTE), "hnh_relu_grad_cols_f64");
        };
        for (int it = 0; it < iters; it++) {
            if (folded_) {
                const hnh_gram_cg cg = {X.data(), r.data(), p.data(), rs.data()};
                apply(p, &cg);
                continue;
            }
            apply(p, nullptr);
            w->check(be->hnh_rowdot_f64(w->ctx, p.data(), Mp.data(), bdot.data(), nrows, R, HNH_STREAM_COMPUTE), "hnh_rowdot_f64");
            w->check(be->hnh_vec_div_f64(w->ctx, quot.data(), rs.data(), bdot.data(), nrows, HNH_STREAM_COMPUTE), "hnh_vec_div_f64");
            select(alpha, quot, bdot);
            w->check(be->hnh_cg_step_f64(w->ctx, X.data(), r.data(), p.data(), Mp.data(), alpha.data(), rsnew.data(), nrows, R, HNH_STREAM_COMPUTE), "hnh_cg_step_f64");
            w->check(be->hnh_vec_div_f64(w->ctx, quot.data(), rsnew.data(), rs.data(), nrows, HNH_STREAM_COMPUTE), "hnh_vec_div_f64");
            select(beta, quot, rs);
            select(quot, beta, bdot);
            w->check(be->hnh_row_scale_add_f64(w->ctx, p.data(), quot.data(), 1.0, r.data(), nullptr, 1.0, nrows, R, HNH_STREAM_COMPUTE), "hnh_row_scale_add_f64");
            std::swap(rs, rsnew);
        }
    }

    void run(int steps, int iters) {
        for (int s = 0; s < steps; s++) {
            half_step(Amat, iters);
            half_step(Bmat, iters);
        }
    }

    // The closed form above: one sddmmA for the s_e, the two Gram matrices (their traces are the norms), and one host all-reduce of
    // the three sums over the stored pairs (the values are downloaded and reduced on the host, as computeResidual does)
    double loss() {
        require_embeddings("loss");
        if (!confidence_set_) throw hnh::Error("Error, Implicit_ALS loss needs set_confidence first!");
        VectorXd ones = d_ops->like_S_values(1.0), s = d_ops->like_S_values(0.0);
        d_ops->sddmmA(A, B, ones, s);
        const std::vector<double> sh = s.to_host();
        double sums[3] = {0.0, 0.0, 0.0};  // sum (1 + w)(1 - s)^2, sum s^2, stored pairs
        for (size_t e = 0; e < sh.size(); e++) {
            sums[0] += (1.0 + w_host_[e]) * (1.0 - sh[e]) * (1.0 - sh[e]);
            sums[1] += sh[e] * sh[e];
            sums[2] += 1.0;
        }
        d_ops->world->host_allreduce_sum(sums, 3);
        const int R = (int)d_ops->R;
        const std::vector<double> ga = gram_of(A, Amat).to_host(), gb = gram_of(B, Bmat).to_host();
        double cross = 0.0, norms = 0.0;
        for (size_t k = 0; k < ga.size(); k++) cross += ga[k] * gb[k];
        for (int k = 0; k < R; k++) norms += ga[(size_t)k * R + k] + gb[(size_t)k * R + k];
        return (sums[0] - sums[1]) + cross + lambda * norms;
    }

    // The first k items of every user of `users` (nq global row numbers, repeats allowed) by <a_u, b_j>, best first: ids_host and
    // scores_host receive nq x k entries, global item ids, the tail (-1, -infinity) where fewer than k items are left.  filter_seen: the
    // items of the user's row of S are never returned (S's pattern is enough: set_confidence is not needed).  COLLECTIVE: every rank passes
    // the same users and receives the same result.  There is no host fallback: a kernel library without include/hnh_topk.h is refused.
    void recommend(const int64_t* users, int64_t nq, int k, bool filter_seen, int64_t* ids_host, double* scores_host) {
        require_embeddings("recommend");
        hnh::World* w = d_ops->world;
        hnh::Backend* be = w->be;
        const int R = (int)d_ops->R;
        if (k < 1 || k > HNH_TOPK_MAX_K)
            throw hnh::Error("Error, Implicit_ALS recommend needs 1 <= k <= HNH_TOPK_MAX_K = " + std::to_string(HNH_TOPK_MAX_K) + ", not k = " + std::to_string(k) + "!");
        if (nq < 0 || (nq > 0 && (users == nullptr || ids_host == nullptr || scores_host == nullptr)))
            throw hnh::Error("Error, Implicit_ALS recommend needs nq >= 0 and its three arrays!");
        for (int64_t q = 0; q < nq; q++)
            if (users[q] < 0 || users[q] >= d_ops->M)
                throw hnh::Error("Error, Implicit_ALS recommend: user " + std::to_string(users[q]) + " is outside [0, M = " + std::to_string(d_ops->M) + ")!");
        if (R > HNH_TOPK_MAX_R)
            throw hnh::Error("Error, Implicit_ALS recommend supports R <= HNH_TOPK_MAX_R = " + std::to_string(HNH_TOPK_MAX_R) + ", not R = " + std::to_string(R) + "!");
        if (be->hnh_topk_rows_f64 == nullptr || be->hnh_topk_rows_f64_workspace == nullptr || be->hnh_topk_merge_f64 == nullptr || be->hnh_take_rows_f64 == nullptr)
            throw hnh::Error(be->missing_kernel("Implicit_ALS recommend", "hnh_topk_rows_f64"));
        if (nq == 0) return;
        const DenseSubmatrix& subA = d_ops->aSubmatrices[0];
        const DenseSubmatrix& subB = d_ops->bSubmatrices[0];
        const int64_t validB = std::max<int64_t>(0, std::min<int64_t>(subB.rowCount, d_ops->N - subB.topRow));

        // the queries' rows of A, the same bits on every rank: each rank gathers the rows it owns into a zeroed matrix, and adding +0.0 is exact
        std::vector<int64_t> idx((size_t)nq);
        for (int64_t q = 0; q < nq; q++) {
            const int64_t local = users[q] - subA.topRow;
            idx[(size_t)q] = (local >= 0 && local < subA.rowCount) ? local : -1;
        }
        DenseMatrix idx_d(nq, 1), Qd(nq, R);  // (idx_d holds int64)
        w->copy(idx_d.data(), idx.data(), (size_t)nq * sizeof(int64_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        w->check(be->hnh_take_rows_f64(w->ctx, A.data(), subA.rowCount, R, reinterpret_cast<const int64_t*>(idx_d.data()), nq, Qd.data(), HNH_STREAM_COMPUTE),
                 "hnh_take_rows_f64");
        w->allreduce_f64(w->world_comm(), Qd.data(), (size_t)(nq * R), HNH_STREAM_COMPUTE);

        // the exclusion lists of this rank's rows of B, as a CSR over the queries
        DenseMatrix excl_ptr_d, excl_idx_d;
        if (filter_seen) {
            std::vector<int64_t> ptr;
            std::vector<int32_t> items;
            seen_lists(users, nq, subB.topRow, validB, ptr, items);
            excl_ptr_d = DenseMatrix(nq + 1, 1);
            excl_idx_d = DenseMatrix((int64_t)(items.size() / 2 + 1), 1);  // (int32, two to a double; never empty)
            w->copy(excl_ptr_d.data(), ptr.data(), ptr.size() * sizeof(int64_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
            if (!items.empty()) w->copy(excl_idx_d.data(), items.data(), items.size() * sizeof(int32_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        }
        w->sync(HNH_STREAM_COMPUTE);  // the host arrays above may go

        // this rank's list, then every rank's, then their merge: [scores | ids] in one buffer, downloaded once
        const int64_t list = nq * k;
        const int p = w->size;
        DenseMatrix mine(2 * list, 1), merged(2 * list, 1);
        const int64_t need = be->hnh_topk_rows_f64_workspace(nq, validB, R, k);
        DenseMatrix work(std::max<int64_t>((need + 7) / 8, 2), 1);
        DenseMatrix& local_out = p > 1 ? mine : merged;
        w->check(be->hnh_topk_rows_f64(w->ctx, Qd.data(), nq, B.data(), validB, R, subB.topRow, filter_seen ? reinterpret_cast<const int64_t*>(excl_ptr_d.data()) : nullptr,
                                       filter_seen ? reinterpret_cast<const int32_t*>(excl_idx_d.data()) : nullptr, k, 0, local_out.data(),
                                       reinterpret_cast<int64_t*>(local_out.data() + list), work.data(), work.size() * 8, HNH_STREAM_COMPUTE),
                 "hnh_topk_rows_f64");
        if (p > 1) {
            DenseMatrix all_s((int64_t)p * list, 1), all_i((int64_t)p * list, 1);
            w->allgather(w->world_comm(), mine.data(), all_s.data(), (size_t)list * sizeof(double), HNH_STREAM_COMPUTE);
            w->allgather(w->world_comm(), mine.data() + list, all_i.data(), (size_t)list * sizeof(int64_t), HNH_STREAM_COMPUTE);
            w->check(be->hnh_topk_merge_f64(w->ctx, all_s.data(), reinterpret_cast<const int64_t*>(all_i.data()), p, nq, k, merged.data(),
                                            reinterpret_cast<int64_t*>(merged.data() + list), HNH_STREAM_COMPUTE),
                     "hnh_topk_merge_f64");
            w->sync(HNH_STREAM_COMPUTE);  // (the gathered lists go out of scope)
        }
        std::vector<double> host((size_t)(2 * list));
        merged.copy_to_host(host.data());
        std::memcpy(scores_host, host.data(), (size_t)list * sizeof(double));
        std::memcpy(ids_host, host.data() + list, (size_t)list * sizeof(int64_t));
    }

    // The exact position of items[i] in users[i]'s full ordering of the items, for n (user, item) pairs in global coordinates (repeats
    // allowed): ranks_host[i] = the number of items that rank before items[i] in the total order of include/hnh_topk.h among the user's
    // candidates other than the item itself, and candidates_host[i] = the number of those candidates plus the item: N, or with filter_seen
    // N - |seen_u \ {item}| (the items of the user's row of S are no candidates, the asked item always is), so 0 <= rank < candidates.
    // For an item the user has not seen this is its index in recommend(user, k = infinity, filter_seen), bit for bit: the target's score
    // (hnh_pair_scores_f64) and the scores it is compared with (hnh_rank_rows_f64) carry the bits that hnh_topk_rows_f64 returns.
    // in_seen_host (or null) receives 1 where filter_seen and the item is in the user's row of S, else 0.
    // Every rank counts over its own valid rows of B; with filter_seen it scores its share of the users' seen items with
    // hnh_pair_scores_f64 and subtracts those that rank before the target (hnh_rank_exclude_f64): the counting kernel searches nothing.
    // The counts are summed over the ranks on the host, as doubles (they stay below 2^53).  COLLECTIVE: every rank passes the same pairs
    // and receives the same arrays, the same integers for every rank count.  There is no host fallback: a kernel library without
    // include/hnh_rank.h is refused.
    void rank_of(const int64_t* users, const int64_t* items, int64_t n, bool filter_seen, int64_t* ranks_host, int64_t* candidates_host,
                 int64_t* in_seen_host = nullptr) {
        require_embeddings("rank_of");
        hnh::World* w = d_ops->world;
        hnh::Backend* be = w->be;
        const int R = (int)d_ops->R;
        if (n < 0 || (n > 0 && (users == nullptr || items == nullptr || ranks_host == nullptr || candidates_host == nullptr)))
            throw hnh::Error("Error, Implicit_ALS rank_of needs n >= 0 and its four arrays!");
        for (int64_t i = 0; i < n; i++) {
            if (users[i] < 0 || users[i] >= d_ops->M)
                throw hnh::Error("Error, Implicit_ALS rank_of: user " + std::to_string(users[i]) + " is outside [0, M = " + std::to_string(d_ops->M) + ")!");
            if (items[i] < 0 || items[i] >= d_ops->N)
                throw hnh::Error("Error, Implicit_ALS rank_of: item " + std::to_string(items[i]) + " is outside [0, N = " + std::to_string(d_ops->N) + ")!");
        }
        if (R > HNH_RANK_MAX_R)
            throw hnh::Error("Error, Implicit_ALS rank_of supports R <= HNH_RANK_MAX_R = " + std::to_string(HNH_RANK_MAX_R) + ", not R = " + std::to_string(R) + "!");
        if (be->hnh_rank_rows_f64 == nullptr || be->hnh_rank_rows_f64_workspace == nullptr || be->hnh_pair_scores_f64 == nullptr ||
            be->hnh_rank_exclude_f64 == nullptr)
            throw hnh::Error(be->missing_kernel("Implicit_ALS rank_of", "hnh_rank_rows_f64"));
        if (be->hnh_take_rows_f64 == nullptr) throw hnh::Error(be->missing_kernel("Implicit_ALS rank_of", "hnh_take_rows_f64"));
        if (n == 0) return;
        const DenseSubmatrix& subA = d_ops->aSubmatrices[0];
        const DenseSubmatrix& subB = d_ops->bSubmatrices[0];
        const int64_t topB = subB.topRow;
        const int64_t validB = std::max<int64_t>(0, std::min<int64_t>(subB.rowCount, d_ops->N - topB));

        // the pairs grouped by user: target slot t holds pair order[t]; a user with more than HNH_RANK_MAX_TARGETS pairs gets several query rows
        std::vector<int64_t> order((size_t)n);
        for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return users[a] < users[b]; });
        std::vector<int64_t> row_user, tgt_ptr(1, 0), tgt_id((size_t)n), pair_q((size_t)n), pair_j((size_t)n);
        for (int64_t t = 0; t < n; t++) {
            const int64_t i = order[(size_t)t];
            if (t == 0 || users[i] != row_user.back() || t - tgt_ptr[tgt_ptr.size() - 2] == HNH_RANK_MAX_TARGETS) {
                row_user.push_back(users[i]);
                tgt_ptr.push_back(t);
            }
            tgt_ptr.back() = t + 1;
            const int64_t local = items[i] - topB;
            tgt_id[(size_t)t] = items[i];
            pair_q[(size_t)t] = (int64_t)row_user.size() - 1;
            pair_j[(size_t)t] = (local >= 0 && local < validB) ? local : -1;  // (an item of another rank scores +0.0 here)
        }
        const int64_t nq = (int64_t)row_user.size();

        // the query rows of A, as in recommend: the same bits on every rank
        std::vector<int64_t> idx((size_t)nq);
        for (int64_t q = 0; q < nq; q++) {
            const int64_t local = row_user[(size_t)q] - subA.topRow;
            idx[(size_t)q] = (local >= 0 && local < subA.rowCount) ? local : -1;
        }
        auto upload = [&](const std::vector<int64_t>& host) {  // (a DenseMatrix that holds int64; never empty)
            DenseMatrix dev(std::max<int64_t>((int64_t)host.size(), 1), 1);
            if (!host.empty()) w->copy(dev.data(), host.data(), host.size() * sizeof(int64_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
            return dev;
        };
        DenseMatrix idx_d = upload(idx), Qd(nq, R);
        w->check(be->hnh_take_rows_f64(w->ctx, A.data(), subA.rowCount, R, reinterpret_cast<const int64_t*>(idx_d.data()), nq, Qd.data(), HNH_STREAM_COMPUTE),
                 "hnh_take_rows_f64");
        w->allreduce_f64(w->world_comm(), Qd.data(), (size_t)(nq * R), HNH_STREAM_COMPUTE);

        // the targets' scores: the rank that holds the item computes it, the others add +0.0 (at most the sign of a zero changes)
        DenseMatrix tgt_ptr_d = upload(tgt_ptr), tgt_id_d = upload(tgt_id), pair_q_d = upload(pair_q), pair_j_d = upload(pair_j), tgt_score(n, 1), counts(n, 1);
        w->check(be->hnh_pair_scores_f64(w->ctx, Qd.data(), nq, B.data(), validB, R, reinterpret_cast<const int64_t*>(pair_q_d.data()),
                                         reinterpret_cast<const int64_t*>(pair_j_d.data()), n, tgt_score.data(), HNH_STREAM_COMPUTE),
                 "hnh_pair_scores_f64");
        w->allreduce_f64(w->world_comm(), tgt_score.data(), (size_t)n, HNH_STREAM_COMPUTE);

        // the count over this rank's valid rows of B (the padding rows are never candidates)
        const int64_t need = be->hnh_rank_rows_f64_workspace(nq, validB, n, 0);
        if (need < 0) throw hnh::Error("Error, Implicit_ALS rank_of: hnh_rank_rows_f64_workspace refuses the shape!");
        DenseMatrix work(std::max<int64_t>((need + 7) / 8, 2), 1);
        w->check(be->hnh_rank_rows_f64(w->ctx, Qd.data(), nq, B.data(), validB, R, topB, tgt_ptr.data(), tgt_score.data(),
                                       reinterpret_cast<const int64_t*>(tgt_id_d.data()), 0, reinterpret_cast<int64_t*>(counts.data()), work.data(),
                                       work.size() * 8, HNH_STREAM_COMPUTE),
                 "hnh_rank_rows_f64");

        // [counts | is the item seen | the user's seen items], this rank's share of each, summed over the ranks below
        std::vector<double> sums((size_t)(3 * n), 0.0);
        if (filter_seen) {
            std::vector<int64_t> ptr;
            std::vector<int32_t> seen;
            seen_lists(row_user.data(), nq, topB, validB, ptr, seen);
            const int64_t ne = (int64_t)seen.size();
            std::vector<int64_t> ex_q((size_t)ne), ex_j((size_t)ne), ex_id((size_t)ne);
            for (int64_t q = 0; q < nq; q++)
                for (int64_t e = ptr[(size_t)q]; e < ptr[(size_t)q + 1]; e++) {
                    ex_q[(size_t)e] = q;
                    ex_j[(size_t)e] = seen[(size_t)e];
                    ex_id[(size_t)e] = topB + seen[(size_t)e];
                }
            if (ne > 0) {
                DenseMatrix ptr_d = upload(ptr), ex_q_d = upload(ex_q), ex_j_d = upload(ex_j), ex_id_d = upload(ex_id), ex_score(ne, 1);
                w->check(be->hnh_pair_scores_f64(w->ctx, Qd.data(), nq, B.data(), validB, R, reinterpret_cast<const int64_t*>(ex_q_d.data()),
                                                 reinterpret_cast<const int64_t*>(ex_j_d.data()), ne, ex_score.data(), HNH_STREAM_COMPUTE),
                         "hnh_pair_scores_f64");
                w->check(be->hnh_rank_exclude_f64(w->ctx, nq, reinterpret_cast<const int64_t*>(ptr_d.data()), ex_score.data(),
                                                  reinterpret_cast<const int64_t*>(ex_id_d.data()), reinterpret_cast<const int64_t*>(tgt_ptr_d.data()),
                                                  tgt_score.data(), reinterpret_cast<const int64_t*>(tgt_id_d.data()),
                                                  reinterpret_cast<int64_t*>(counts.data()), HNH_STREAM_COMPUTE),
                         "hnh_rank_exclude_f64");
                w->sync(HNH_STREAM_COMPUTE);  // (the uploaded lists go out of scope)
            }
            for (int64_t q = 0; q < nq; q++) {
                const int32_t* first = seen.data() + ptr[(size_t)q];
                const int32_t* last = seen.data() + ptr[(size_t)q + 1];
                for (int64_t t = tgt_ptr[(size_t)q]; t < tgt_ptr[(size_t)q + 1]; t++) {
                    const int64_t j = pair_j[(size_t)t];
                    sums[(size_t)(n + t)] = (j >= 0 && std::binary_search(first, last, (int32_t)j)) ? 1.0 : 0.0;
                    sums[(size_t)(2 * n + t)] = (double)(last - first);
                }
            }
        }
        std::vector<double> got((size_t)n);
        counts.copy_to_host(got.data());  // (int64 in a DenseMatrix; waits for the stream: the host arrays above may go)
        for (int64_t t = 0; t < n; t++) {
            int64_t c;
            std::memcpy(&c, &got[(size_t)t], sizeof(c));
            sums[(size_t)t] = (double)c;
        }
        w->host_allreduce_sum(sums.data(), sums.size());
        for (int64_t t = 0; t < n; t++) {
            const int64_t i = order[(size_t)t];
            const int64_t in_seen = (int64_t)std::llround(sums[(size_t)(n + t)]);
            ranks_host[i] = (int64_t)std::llround(sums[(size_t)t]);
            candidates_host[i] = d_ops->N - ((int64_t)std::llround(sums[(size_t)(2 * n + t)]) - in_seen);
            if (in_seen_host != nullptr) in_seen_host[i] = in_seen;
        }
    }

private:
    VectorXd w_S_, w_ST_, c_S_, c_ST_;
    std::vector<int64_t> seen_rows_, seen_cols_;  // global coordinates of this rank's stored pairs (like_S_values order), read once
    bool seen_cached_ = false;

    // The global coordinates of the local stored pairs: sddmmA of (row id in column 0) against (1 in column 0) gives every pair its row,
    // and the other way round its column (ids are exact in fp64).  Cached: S's pattern never changes.
    void cache_seen_coordinates() {
        if (seen_cached_) return;
        const int64_t R = d_ops->R;
        DenseMatrix PA = d_ops->like_A_matrix(0.0), PB = d_ops->like_B_matrix(0.0);
        VectorXd ones = d_ops->like_S_values(1.0), s = d_ops->like_S_values(0.0);
        std::vector<double> ha((size_t)(PA.rows() * R), 0.0), hb((size_t)(PB.rows() * R), 0.0);
        const int64_t topA = d_ops->aSubmatrices[0].topRow, topB = d_ops->bSubmatrices[0].topRow;
        for (int pass = 0; pass < 2; pass++) {
            for (int64_t i = 0; i < PA.rows(); i++) ha[(size_t)(i * R)] = pass == 0 ? (double)(topA + i) : 1.0;
            for (int64_t j = 0; j < PB.rows(); j++) hb[(size_t)(j * R)] = pass == 0 ? 1.0 : (double)(topB + j);
            PA.copy_from_host(ha.data());
            PB.copy_from_host(hb.data());
            d_ops->sddmmA(PA, PB, ones, s);
            const std::vector<double> got = s.to_host();
            std::vector<int64_t>& dst = pass == 0 ? seen_rows_ : seen_cols_;
            dst.resize(got.size());
            for (size_t e = 0; e < got.size(); e++) dst[e] = (int64_t)std::llround(got[e]);
        }
        seen_cached_ = true;
    }

    // ptr / items: for every query q the rows j - topB of this rank's valid B rows whose item j the user has seen, ascending and without
    // repeats.  With c > 1 a rank's block of S is not aligned with its rows of B, so the (query, item) pairs of all ranks are exchanged:
    // one round of counts, one padded round of payload.
    void seen_lists(const int64_t* users, int64_t nq, int64_t topB, int64_t validB, std::vector<int64_t>& ptr, std::vector<int32_t>& items) {
        cache_seen_coordinates();
        hnh::World* w = d_ops->world;
        std::unordered_map<int64_t, std::vector<int64_t>> queries_of;  // a user may be asked for more than once
        for (int64_t q = 0; q < nq; q++) queries_of[users[q]].push_back(q);
        std::vector<int64_t> pairs;  // (query, item), ...
        for (size_t e = 0; e < seen_rows_.size(); e++) {
            auto it = queries_of.find(seen_rows_[e]);
            if (it == queries_of.end()) continue;
            for (int64_t q : it->second) {
                pairs.push_back(q);
                pairs.push_back(seen_cols_[e]);
            }
        }
        const int p = w->size;
        std::vector<int64_t> counts((size_t)p, 0);
        const int64_t my_count = (int64_t)pairs.size();
        w->host_allgather(&my_count, counts.data(), sizeof(int64_t));
        const int64_t widest = *std::max_element(counts.begin(), counts.end());
        std::vector<int64_t> all((size_t)p * (size_t)widest, 0);
        if (widest > 0) {
            pairs.resize((size_t)widest, 0);
            w->host_allgather(pairs.data(), all.data(), (size_t)widest * sizeof(int64_t));
        }
        std::vector<std::pair<int64_t, int64_t>> mine;
        for (int r = 0; r < p; r++)
            for (int64_t x = 0; x + 1 < counts[(size_t)r]; x += 2) {
                const int64_t q = all[(size_t)r * (size_t)widest + (size_t)x], j = all[(size_t)r * (size_t)widest + (size_t)x + 1] - topB;
                if (j >= 0 && j < validB) mine.emplace_back(q, j);
            }
        std::sort(mine.begin(), mine.end());
        mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
        ptr.assign((size_t)nq + 1, 0);
        items.clear();
        for (const auto& qj : mine) {
            ptr[(size_t)qj.first + 1]++;
            items.push_back((int32_t)qj.second);
        }
        for (int64_t q = 0; q < nq; q++) ptr[(size_t)q + 1] += ptr[(size_t)q];
    }

    std::vector<double> w_host_;  // w in the like_S_values layout, for loss()
    bool confidence_set_ = false, folded_ = false;

    void require_embeddings(const char* who) const {
        if (A.rows() != d_ops->localArows || B.rows() != d_ops->localBrows || A.cols() != d_ops->R || B.cols() != d_ops->R)
            throw hnh::Error(std::string("Error, Implicit_ALS ") + who + " needs initializeEmbeddings or set_embeddings first (at the operator's R)!");
    }

    // X^T X over this rank's VALID rows (the padding rows past M or N contribute nothing), summed over all ranks in the all-reduce's
    // fixed order: hnh_gemm_tn_f64 with X as both operands
    DenseMatrix gram_of(const DenseMatrix& X, MatMode which) {
        hnh::World* w = d_ops->world;
        hnh::Backend* be = w->be;
        if (be->hnh_gemm_tn_f64 == nullptr || be->hnh_gemm_tn_f64_workspace == nullptr)
            throw hnh::Error(be->missing_kernel("Implicit_ALS", "hnh_gemm_tn_f64"));
        const int64_t R = d_ops->R;
        const DenseSubmatrix& sub = (which == Amat ? d_ops->aSubmatrices : d_ops->bSubmatrices)[0];
        const int64_t total = which == Amat ? d_ops->M : d_ops->N;
        const int64_t valid = std::max<int64_t>(0, std::min<int64_t>(sub.rowCount, total - sub.topRow));
        DenseMatrix G(R, R);
        if (valid == 0) {
            G.setZero();
        } else {
            const int64_t need = be->hnh_gemm_tn_f64_workspace(R, R, valid);
            DenseMatrix work(std::max<int64_t>(need, 1), 1);
            w->check(be->hnh_gemm_tn_f64(w->ctx, R, R, valid, X.data(), R, X.data(), R, G.data(), R, need > 0 ? work.data() : nullptr, need, HNH_STREAM_COMPUTE),
                     "hnh_gemm_tn_f64");
        }
        w->allreduce_f64(w->world_comm(), G.data(), (size_t)(R * R), HNH_STREAM_COMPUTE);
        return G;
    }

    void hashed_fill(DenseMatrix& loc, MatMode mode, uint64_t fill_seed, double scale) {
        std::vector<DenseSubmatrix>& subs = (mode == Amat) ? d_ops->aSubmatrices : d_ops->bSubmatrices;
        hnh::World* w = d_ops->world;
        double* ptr = loc.data();
        for (auto& s : subs) {
            w->check(w->be->hnh_fill_hashed_f64(w->ctx, ptr, s.rowCount, s.colCount, s.topRow, s.leftCol, d_ops->R, fill_seed, scale, HNH_STREAM_COMPUTE),
                     "hnh_fill_hashed_f64");
            ptr += (size_t)s.rowCount * s.colCount;
        }
    }
};
