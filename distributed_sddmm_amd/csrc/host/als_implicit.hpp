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
#pragma once
#include <cmath>
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

private:
    VectorXd w_S_, w_ST_, c_S_, c_ST_;
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
