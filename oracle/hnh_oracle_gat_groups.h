/*
 * TEST INFRASTRUCTURE ONLY — four OPTIONAL groups of the kernel ABI restated in plain C for the second CPU test double
 * (oracle/liboracle_backend_gat.so = hnh_oracle_backend.c compiled with -DHNH_ORACLE_GAT_GROUPS, which includes this file at its end):
 *   include/hnh_grad.h       hnh_gemm_tn_f64(_workspace), hnh_leaky_relu_grad_f64, hnh_relu_grad_cols_f64, hnh_act_grad_cols_f64,
 *                            hnh_sum3_cols_f64, hnh_transpose_into_f64
 *   include/hnh_attention.h  hnh_attn_softmax_csr_p, hnh_softmax_gate_f64, hnh_rowdot_cols_f64
 *   include/hnh_attn_grad.h  hnh_attn_grad_row_csr_p, hnh_attn_grad_col_csr_p, hnh_attn_grad_pack_f64
 *   include/hnh_train.h      hnh_xent_rows_f64(_workspace), hnh_optim_step_f64
 * so that GAT::backwardPass, the softmax pipeline on the auxiliary stream, attn_walk and the training step run under the stream-order
 * checker (hnh_stream_order.h).  liboracle_backend.so (without the flag) stays the mandatory table alone: the host layer's "missing
 * symbol" refusals are tested against it.
 *
 * The headers are the specification; the argument checks return what the HIP entry points return (csrc/hip/hnh_grad.hip,
 * hnh_kernels.hip, hnh_attn_grad_kernels.hpp, hnh_train_kernels.hpp) and a refused call writes nothing.  The arithmetic is the headers'
 * formulas in their simplest order (one accumulator per sum, nonzero by nonzero): not the kernels' rounding, only their definition.
 *
 * Declarations to the checker: a call opens with HB_OP and names the exact bytes it touches.
 *   - an operand with a pitch wider than its width is declared row by row (ga_rows), never as rows * pitch: the columns between belong
 *     to other heads, which other streams may be writing;
 *   - a gathered operand is declared from the first to the last row its column indices address (the span hb_row_pass declares), ending
 *     with that row's last column in use;
 *   - an output the call overwrites is declared as a write only, one it continues as a read and a write;
 *   - workspaces are declared at the size the _workspace function names (the host sizes its buffers by it);
 *   - a call whose declarations run past the end of a block is reported (MISUSE) and refused, not performed (GA_PERFORM).
 * hnh_attn_softmax_csr_p refuses HNH_ATTN_ADDEND as an unknown flag: include/hnh_gat_skip.h ties that bit to a library that exports
 * hnh_skip_grad_cols_f64, which this one does not.
 */
#include <math.h>

#include "hnh_attention.h"
#include "hnh_attn_grad.h"
#include "hnh_gat_skip.h" /* HNH_ATTN_ADDEND: named to be refused */
#include "hnh_grad.h"
#include "hnh_train.h"

/* rows x cols doubles at pitch ld */
static void ga_rows(const double* p, int64_t ld, int64_t rows, int64_t cols, int write) {
    if (hb_cur.depth <= 0 || !p || rows <= 0 || cols <= 0) return;
    if (ld == cols) { hb_access_at(p, (size_t)rows * (size_t)cols * sizeof(double), write, 1); return; }
    for (int64_t r = 0; r < rows; r++) hb_access_at(p + r * ld, (size_t)cols * sizeof(double), write, 1);
}
#define GA_R(p, ld, rows, cols) ga_rows((p), (ld), (rows), (cols), 0)
#define GA_W(p, ld, rows, cols) ga_rows((p), (ld), (rows), (cols), 1)
/* an output: continued (read and write) or overwritten (write only) */
#define GA_OUT(p, ld, rows, cols, overwrite) do { if (!(overwrite)) GA_R(p, ld, rows, cols); GA_W(p, ld, rows, cols); } while (0)

/* Behind a call's declarations: one that ran past the end of a block has been reported as MISUSE, and is NOT performed — on the host it
 * would write into the heap behind the block, on the GPU it faults.  The caller sees HNH_ERR_INVALID instead of a crash later on. */
#define GA_PERFORM(c, who)                                                                                                  \
    do {                                                                                                                    \
        if (hb_cur.depth > 0 && hb_cur.overrun)                                                                             \
            return ga_fail((c), HNH_ERR_INVALID, (who), "an operand runs past the end of its device block (the checker's MISUSE report names it): not performed"); \
    } while (0)

static int ga_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static int ga_fail(hnh_ctx* c, int code, const char* who, const char* what) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fail(c, code, msg);
}

/* the index streams and the values of a pass over [beg[r], end[r]) of every row, and `width` columns of the rows of `gathered` (pitch
 * ld) from the first to the last the column indices address */
static void ga_row_pass(const hnh_csr_block* b, const hnh_csr_window* w, const double* values, int values_overwrite, const double* gathered, int64_t ld,
                        int64_t width) {
    if (hb_cur.depth <= 0 || b->rows <= 0) return;
    const int32_t *beg = w ? w->beg : NULL, *end = w ? w->end : NULL;
    hb_row_pass(b->rows, b->rowptr, b->col_idx, beg, end, NULL, -1, NULL, NULL, 0);
    int64_t lo = -1, hi = -1;
    int32_t cmin = 0, cmax = 0;
    for (int64_t r = 0; r < b->rows; r++) {
        const int32_t s = beg ? beg[r] : b->rowptr[r], e = end ? end[r] : b->rowptr[r + 1];
        if (s >= e) continue;
        if (lo < 0) { lo = s; hi = e; cmin = cmax = b->col_idx[s]; }
        if (s < lo) lo = s;
        if (e > hi) hi = e;
        for (int32_t i = s; i < e; i++) {
            if (b->col_idx[i] < cmin) cmin = b->col_idx[i];
            if (b->col_idx[i] > cmax) cmax = b->col_idx[i];
        }
    }
    if (lo < 0) return;
    if (values) {
        if (!values_overwrite) HB_R(values + lo, (size_t)(hi - lo) * sizeof(double));
        HB_W(values + lo, (size_t)(hi - lo) * sizeof(double));
    }
    if (gathered) HB_R(gathered + (int64_t)cmin * ld, (size_t)((int64_t)(cmax - cmin) * ld + width) * sizeof(double));
}

/* ------------------------------------------------------------------------------------------------ include/hnh_grad.h */
/* the K split of csrc/hip/hnh_grad.hip (tn_plan): 128 x 128 tiles, 16-row K tiles, up to 64 slices of at least 32 K tiles that bring the
 * launch to 512 workgroups; it sizes the workspace, so it is restated with its constants */
static int64_t ga_tn_slices(int64_t M, int64_t N, int64_t K, int64_t* kc) {
    const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128), kt = (K + 15) / 16;
    int64_t s = 1;
    if (tiles > 0 && tiles < 512) {
        s = (512 + tiles - 1) / tiles;
        if (s > kt / 32) s = kt / 32;
        if (s > 64) s = 64;
        if (s < 1) s = 1;
    }
    const int64_t per = kt > 0 ? (kt + s - 1) / s : 1;
    if (kc) *kc = per * 16;
    return kt > 0 ? (kt + per - 1) / per : 1;
}
int64_t hnh_gemm_tn_f64_workspace(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int64_t s = ga_tn_slices(M, N, K, NULL);
    return s > 1 ? s * M * N : 0;
}
int hnh_gemm_tn_f64(hnh_ctx* c, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                    int64_t ldc, double* work, int64_t work_doubles, int stream) {
    const char* who = "hnh_gemm_tn_f64";
    if (M < 0 || N < 0 || K < 0) return ga_fail(c, HNH_ERR_INVALID, who, "negative size");
    if (lda < M || ldb < N || ldc < N) return ga_fail(c, HNH_ERR_INVALID, who, "leading dimension smaller than the width");
    if (M == 0 || N == 0) return HNH_OK;
    if (!C) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    if (K > 0 && (!A || !B)) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    int64_t kc = 0;
    const int64_t slices = K > 0 ? ga_tn_slices(M, N, K, &kc) : 1, need = slices > 1 ? slices * M * N : 0;
    if (need > 0 && (!work || work_doubles < need)) return ga_fail(c, HNH_ERR_INVALID, who, "workspace smaller than hnh_gemm_tn_f64_workspace()");
    HB_OP(c, stream, "hnh_gemm_tn_f64");
    GA_R(A, lda, K, M);
    GA_R(B, ldb, K, N);
    GA_W(C, ldc, M, N);
    if (need > 0) HB_W(work, (size_t)need * sizeof(double));
    GA_PERFORM(c, who);
    for (int64_t i = 0; i < M; i++)
        for (int64_t j = 0; j < N; j++) C[i * ldc + j] = 0.0;
    /* every slice's partial product into its slab, then the slabs in slice order (one slice: straight into C) */
    for (int64_t s = 0; s < slices && K > 0; s++) {
        double* dst = need > 0 ? work + s * M * N : C;
        const int64_t ld = need > 0 ? N : ldc, k1 = (s + 1) * kc < K ? (s + 1) * kc : K;
        if (need > 0) memset(dst, 0, sizeof(double) * (size_t)(M * N));
        for (int64_t k = s * kc; k < k1; k++)
            for (int64_t i = 0; i < M; i++) {
                const double a = A[k * lda + i];
                for (int64_t j = 0; j < N; j++) dst[i * ld + j] += a * B[k * ldb + j];
            }
    }
    for (int64_t s = 0; s < slices && need > 0; s++)
        for (int64_t i = 0; i < M; i++)
            for (int64_t j = 0; j < N; j++) C[i * ldc + j] += work[s * M * N + i * N + j];
    return HNH_OK;
}

int hnh_leaky_relu_grad_f64(hnh_ctx* c, double* e_to_a, double* da_to_de, double alpha, int64_t n, int stream) {
    const char* who = "hnh_leaky_relu_grad_f64";
    if (n < 0) return ga_fail(c, HNH_ERR_INVALID, who, "negative size");
    if (n == 0) return HNH_OK;
    if (!e_to_a || !da_to_de) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_leaky_relu_grad_f64");
    GA_OUT(e_to_a, n, 1, n, 0);
    GA_OUT(da_to_de, n, 1, n, 0);
    GA_PERFORM(c, who);
    for (int64_t i = 0; i < n; i++) {
        const double x = e_to_a[i];
        e_to_a[i] = (x > 0.0 ? x : 0.0) + (x < 0.0 ? x : 0.0) * alpha;  /* hnh_leaky_relu_f64's activation */
        da_to_de[i] = x > 0.0 ? da_to_de[i] : da_to_de[i] * alpha;
    }
    return HNH_OK;
}

int hnh_relu_grad_cols_f64(hnh_ctx* c, double* dZ, int64_t ld_dz, const double* G, int64_t ld_g, const double* out, int64_t ld_out, int64_t col0,
                           int64_t rows, int64_t cols, int stream) {
    const char* who = "hnh_relu_grad_cols_f64";
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || col0 + cols > ld_g || col0 + cols > ld_out) return ga_fail(c, HNH_ERR_INVALID, who, "bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dZ || !G || !out) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_relu_grad_cols_f64");
    GA_R(G + col0, ld_g, rows, cols);
    GA_R(out + col0, ld_out, rows, cols);
    GA_W(dZ, ld_dz, rows, cols);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t j = 0; j < cols; j++) dZ[r * ld_dz + j] = out[r * ld_out + col0 + j] > 0.0 ? G[r * ld_g + col0 + j] : 0.0;
    return HNH_OK;
}

int hnh_act_grad_cols_f64(hnh_ctx* c, double* dZ, int64_t ld_dz, double* delta, const double* G, int64_t ld_g, const double* out, int64_t ld_out,
                          int64_t col0, int64_t rows, int64_t cols, int act, int stream) {
    const char* who = "hnh_act_grad_cols_f64";
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || col0 + cols > ld_g || col0 + cols > ld_out || cols > 0x7fffffffLL)
        return ga_fail(c, HNH_ERR_INVALID, who, "bad shape");
    if (act != HNH_ACT_RELU && act != HNH_ACT_ELU && act != HNH_ACT_IDENTITY) return ga_fail(c, HNH_ERR_INVALID, who, "unknown activation (relu = 0, elu = 1, identity = 2)");
    if (rows == 0) return HNH_OK;
    if (!delta || (cols > 0 && (!dZ || !G || !out))) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_act_grad_cols_f64");
    GA_R(G + col0, ld_g, rows, cols);
    GA_R(out + col0, ld_out, rows, cols);
    GA_W(dZ, ld_dz, rows, cols);
    GA_W(delta, rows, 1, rows);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++) {
        double s = 0.0;
        for (int64_t j = 0; j < cols; j++) {
            const double o = out[r * ld_out + col0 + j], g = G[r * ld_g + col0 + j];
            double z;
            if (act == HNH_ACT_RELU) {
                z = o > 0.0 ? g : 0.0;
                s += z * o;
            } else if (act == HNH_ACT_IDENTITY || o >= 0.0) {
                z = g;
                s += g * o;
            } else {
                const double u = 1.0 + o;
                z = g * u;
                if (u > 0.0) s += z * log1p(o);  /* a unit saturated at -1: dZ = 0 and no term */
            }
            dZ[r * ld_dz + j] = z;
        }
        delta[r] = s;
    }
    return HNH_OK;
}

int hnh_sum3_cols_f64(hnh_ctx* c, double* dst, int64_t ld_dst, int64_t col0, const double* x, const double* y, const double* z, int64_t rows,
                      int64_t cols, int stream) {
    const char* who = "hnh_sum3_cols_f64";
    if (rows < 0 || cols < 0 || col0 < 0 || col0 + cols > ld_dst) return ga_fail(c, HNH_ERR_INVALID, who, "bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst || !x || !y || !z) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_sum3_cols_f64");
    GA_R(x, cols, rows, cols);
    GA_R(y, cols, rows, cols);
    GA_R(z, cols, rows, cols);
    GA_W(dst + col0, ld_dst, rows, cols);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t j = 0; j < cols; j++) dst[r * ld_dst + col0 + j] = (x[r * cols + j] + y[r * cols + j]) + z[r * cols + j];
    return HNH_OK;
}

int hnh_transpose_into_f64(hnh_ctx* c, double* dst, int64_t ld_dst, int64_t row0, const double* W, int64_t rows, int64_t cols, int stream) {
    const char* who = "hnh_transpose_into_f64";
    if (rows < 0 || cols < 0 || row0 < 0 || ld_dst < rows) return ga_fail(c, HNH_ERR_INVALID, who, "bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst || !W) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_transpose_into_f64");
    GA_R(W, cols, rows, cols);
    GA_W(dst + row0 * ld_dst, ld_dst, cols, rows);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t j = 0; j < cols; j++) dst[(row0 + j) * ld_dst + r] = W[r * cols + j];
    return HNH_OK;
}

/* ------------------------------------------------------------------------------------------------ include/hnh_attention.h */
int hnh_attn_softmax_csr_p(hnh_ctx* c, const hnh_csr_block* b, double* values, const double* X, const double* Y, double* Out, int R, unsigned flags,
                           const hnh_attn_state* st, const hnh_csr_window* w, int stream) {
    const char* who = "hnh_attn_softmax_csr_p";
    const unsigned acts = HNH_ATTN_ACT_ELU | HNH_ATTN_ACT_IDENTITY;
    if (!b || !st) return ga_fail(c, HNH_ERR_INVALID, who, "null block or state");
    if (b->rows < 0) return ga_fail(c, HNH_ERR_INVALID, who, "negative size");
    if (R <= 0) return ga_fail(c, HNH_ERR_INVALID, who, "R must be positive");
    if (flags & HNH_ATTN_ADDEND) return ga_fail(c, HNH_ERR_INVALID, who, "unknown flag (HNH_ATTN_ADDEND belongs to a library that exports hnh_skip_grad_cols_f64)");
    if (flags & ~(HNH_FUSED_VALUES_OVERWRITE | HNH_FUSED_OUT_OVERWRITE | HNH_ATTN_FINISH | acts)) return ga_fail(c, HNH_ERR_INVALID, who, "unknown flag");
    const int finish = (flags & HNH_ATTN_FINISH) != 0, fresh = (flags & HNH_FUSED_OUT_OVERWRITE) != 0;
    if ((flags & acts) == acts) return ga_fail(c, HNH_ERR_INVALID, who, "HNH_ATTN_ACT_ELU and HNH_ATTN_ACT_IDENTITY exclude each other");
    if ((flags & acts) && !finish) return ga_fail(c, HNH_ERR_INVALID, who, "an activation flag needs HNH_ATTN_FINISH");
    if (finish && w && !w->last) return ga_fail(c, HNH_ERR_INVALID, who, "the finish belongs to the last window");
    if (!st->row_max || !st->row_sum || !st->lse || !st->relu_dst) return ga_fail(c, HNH_ERR_INVALID, who, "null state pointer");
    if (st->relu_ld < R) return ga_fail(c, HNH_ERR_INVALID, who, "relu_ld is narrower than R");
    const int64_t rows = b->rows;
    if (rows == 0) return HNH_OK;
    if (!Out) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    if (!b->rowptr) {
        if (b->nnz > 0) return ga_fail(c, HNH_ERR_INVALID, who, "null rowptr");
    } else {
        if (!b->col_idx || !values || !X || !Y) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
        if (X == Out || Y == Out) return ga_fail(c, HNH_ERR_INVALID, who, "Out aliases an input");
        const int wide = R % 2 == 0 && ga_aligned16(X) && ga_aligned16(Y) && ga_aligned16(Out) && ga_aligned16(st->relu_dst) && st->relu_ld % 2 == 0;
        if (R > (wide ? 512 : 256))
            return ga_fail(c, HNH_ERR_UNSUPPORTED, who, "width beyond the one-pass instances (R <= 512 even with 16-byte aligned operands and an even relu_ld, R <= 256 otherwise)");
    }
    HB_OP(c, stream, "hnh_attn_softmax_csr_p");
    if (b->rowptr) {
        ga_row_pass(b, w, values, (flags & HNH_FUSED_VALUES_OVERWRITE) != 0, Y, R, R);
        GA_R(X, R, rows, R);
    }
    /* a block without nonzeros that neither resets nor finishes still rewrites the state it read: the bytes do not change, and it is
     * declared as what the kernel does */
    GA_OUT(Out, R, rows, R, fresh);
    GA_OUT(st->row_max, rows, 1, rows, fresh);
    GA_OUT(st->row_sum, rows, 1, rows, fresh);
    if (finish) {
        GA_W(st->lse, rows, 1, rows);
        GA_W(st->relu_dst, st->relu_ld, rows, R);
    }
    GA_PERFORM(c, who);
    const double alpha = st->leaky_alpha;
    for (int64_t r = 0; r < rows; r++) {
        double m = fresh ? -INFINITY : st->row_max[r], l = fresh ? 0.0 : st->row_sum[r];
        double* acc = Out + r * R;
        if (fresh)
            for (int k = 0; k < R; k++) acc[k] = 0.0;
        const int32_t lo = !b->rowptr ? 0 : (w && w->beg ? w->beg[r] : b->rowptr[r]), hi = !b->rowptr ? 0 : (w && w->end ? w->end[r] : b->rowptr[r + 1]);
        for (int32_t e = lo; e < hi; e++) {
            const double* y = Y + (int64_t)R * b->col_idx[e];
            double dot = 0.0;
            for (int k = 0; k < R; k++) dot += X[r * R + k] * y[k];
            if (!(flags & HNH_FUSED_VALUES_OVERWRITE)) dot += values[e];
            const double s = dot > 0.0 ? dot : alpha * dot;
            values[e] = s;
            const double nm = s > m ? s : m;
            const double f = nm == m ? 1.0 : (m == -INFINITY ? 0.0 : exp(m - nm)), p = exp(s - nm);
            if (f != 1.0) {
                for (int k = 0; k < R; k++) acc[k] *= f;
                l *= f;
            }
            l += p;
            for (int k = 0; k < R; k++) acc[k] += p * y[k];
            m = nm;
        }
        st->row_max[r] = m;
        st->row_sum[r] = l;
        if (finish) {
            for (int k = 0; k < R; k++) {
                const double o = l > 0.0 ? acc[k] / l : 0.0;
                double v;
                if (!(l > 0.0)) v = 0.0;
                else if (flags & HNH_ATTN_ACT_IDENTITY) v = o;
                else if (flags & HNH_ATTN_ACT_ELU) v = o > 0.0 ? o : expm1(o);
                else v = o > 0.0 ? o : 0.0;
                st->relu_dst[r * st->relu_ld + k] = v;
            }
            st->lse[r] = l > 0.0 ? m + log(l) : 0.0;
        }
    }
    return HNH_OK;
}

int hnh_softmax_gate_f64(hnh_ctx* c, double* e_to_a, double* da_to_de, const double* lse, const double* delta, double alpha, int64_t n, int stream) {
    const char* who = "hnh_softmax_gate_f64";
    if (n < 0) return ga_fail(c, HNH_ERR_INVALID, who, "bad size");
    if (n == 0) return HNH_OK;
    if (!e_to_a || !da_to_de || !lse || !delta) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_softmax_gate_f64");
    GA_R(lse, n, 1, n);
    GA_R(delta, n, 1, n);
    GA_OUT(e_to_a, n, 1, n, 0);
    GA_OUT(da_to_de, n, 1, n, 0);
    GA_PERFORM(c, who);
    for (int64_t i = 0; i < n; i++) {
        const double e = e_to_a[i], a = exp((e > 0.0 ? e : alpha * e) - lse[i]);
        e_to_a[i] = a;
        da_to_de[i] = a * (da_to_de[i] - delta[i]) * (e > 0.0 ? 1.0 : alpha);
    }
    return HNH_OK;
}

int hnh_rowdot_cols_f64(hnh_ctx* c, double* out, const double* dZ, int64_t ld_dz, const double* O, int64_t ld_o, int64_t col0, int64_t rows,
                        int64_t cols, int stream) {
    const char* who = "hnh_rowdot_cols_f64";
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || ld_o < col0 + cols) return ga_fail(c, HNH_ERR_INVALID, who, "bad size");
    if (rows == 0) return HNH_OK;
    if (!out || !dZ || !O) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_rowdot_cols_f64");
    GA_R(dZ, ld_dz, rows, cols);
    GA_R(O + col0, ld_o, rows, cols);
    GA_W(out, rows, 1, rows);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++) {
        double s = 0.0;
        for (int64_t j = 0; j < cols; j++) s += dZ[r * ld_dz + j] * O[r * ld_o + col0 + j];
        out[r] = s;
    }
    return HNH_OK;
}

/* ------------------------------------------------------------------------------------------------ include/hnh_attn_grad.h */
static int ga_attn_grad(hnh_ctx* c, const hnh_csr_block* b, const hnh_attn_grad* g, unsigned flags, const hnh_csr_window* w, int stream, int col_pass,
                        const char* who) {
    if (!b || !g) return ga_fail(c, HNH_ERR_INVALID, who, "null block or arguments");
    if (b->rows < 0) return ga_fail(c, HNH_ERR_INVALID, who, "negative size");
    if (g->f <= 0) return ga_fail(c, HNH_ERR_INVALID, who, "R must be positive");
    if (flags & ~HNH_FUSED_OUT_OVERWRITE) return ga_fail(c, HNH_ERR_INVALID, who, "unknown flag");
    if (g->f > HNH_ATTN_GRAD_MAX_F) return ga_fail(c, HNH_ERR_UNSUPPORTED, who, "head width beyond the limit of HNH_ATTN_GRAD_MAX_F");
    const int64_t rows = b->rows;
    if (rows == 0) return HNH_OK;
    const int f = g->f, fp = f + (f & 1), overwrite = (flags & HNH_FUSED_OUT_OVERWRITE) != 0;
    const int softmax = col_pass ? (g->softmax != 0) : (g->lse != NULL);
    const int64_t pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax);
    if (!g->Out || g->ld_out < f) return ga_fail(c, HNH_ERR_INVALID, who, "bad output");
    if (!b->rowptr) {  /* a block without nonzeros: an overwriting call stores zeros */
        if (b->nnz > 0) return ga_fail(c, HNH_ERR_INVALID, who, "null rowptr");
        if (!overwrite) return HNH_OK;
        HB_OP(c, stream, who);
        GA_W(g->Out, g->ld_out, rows, f);
    GA_PERFORM(c, who);
        for (int64_t r = 0; r < rows; r++)
            for (int k = 0; k < f; k++) g->Out[r * g->ld_out + k] = 0.0;
        return HNH_OK;
    }
    if (!b->col_idx || !g->X || !g->Y) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    if (g->ld_x < f) return ga_fail(c, HNH_ERR_INVALID, who, "ld_x is narrower than f");
    if (g->X == g->Out || g->Y == g->Out) return ga_fail(c, HNH_ERR_INVALID, who, "Out aliases an input");
    if (!col_pass) {
        if (!g->dZ || g->ld_dz < f || g->ld_y < f) return ga_fail(c, HNH_ERR_INVALID, who, "bad dZ or gathered operand");
        if ((g->lse == NULL) != (g->delta == NULL)) return ga_fail(c, HNH_ERR_INVALID, who, "lse and delta go together");
        if (g->dZ == g->Out) return ga_fail(c, HNH_ERR_INVALID, who, "Out aliases an input");
    } else if (g->ld_y < pw || g->ld_y % 2 != 0 || !ga_aligned16(g->Y)) {
        return ga_fail(c, HNH_ERR_INVALID, who, "the packed operand needs an even pitch of at least the packed width and a 16-byte aligned base");
    }
    HB_OP(c, stream, who);
    ga_row_pass(b, w, NULL, 0, g->Y, g->ld_y, col_pass ? pw : f);
    GA_R(g->X, g->ld_x, rows, f);
    if (!col_pass) {
        GA_R(g->dZ, g->ld_dz, rows, f);
        if (softmax) {
            GA_R(g->lse, rows, 1, rows);
            GA_R(g->delta, rows, 1, rows);
        }
    }
    GA_OUT(g->Out, g->ld_out, rows, f, overwrite);
    GA_PERFORM(c, who);
    const double alpha = g->leaky_alpha;
    for (int64_t r = 0; r < rows; r++) {
        double* acc = g->Out + r * g->ld_out;
        const double* x = g->X + r * g->ld_x;
        if (overwrite)
            for (int k = 0; k < f; k++) acc[k] = 0.0;
        const int32_t lo = w && w->beg ? w->beg[r] : b->rowptr[r], hi = w && w->end ? w->end[r] : b->rowptr[r + 1];
        for (int32_t e = lo; e < hi; e++) {
            const double* y = g->Y + (int64_t)b->col_idx[e] * g->ld_y;
            /* row pass: the row's own dZ against the gathered A_j; column pass: the row's A_j against the gathered dZ_i (packed) */
            const double* left = col_pass ? x : g->dZ + r * g->ld_dz;
            const double* right = col_pass ? y + fp : y;
            double ev = 0.0, da = 0.0;
            for (int k = 0; k < f; k++) {
                ev += x[k] * y[k];
                da += left[k] * right[k];
            }
            const double gate = ev > 0.0 ? 1.0 : alpha, s = ev > 0.0 ? ev : alpha * ev;
            double a = s, de = da * gate;
            if (softmax) {
                const double lse = col_pass ? y[2 * fp] : g->lse[r], delta = col_pass ? y[2 * fp + 1] : g->delta[r];
                a = exp(s - lse);
                de = a * (da - delta) * gate;
            }
            if (col_pass)
                for (int k = 0; k < f; k++) acc[k] += a * y[fp + k] + de * y[k];
            else
                for (int k = 0; k < f; k++) acc[k] += de * y[k];
        }
    }
    return HNH_OK;
}
int hnh_attn_grad_row_csr_p(hnh_ctx* c, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* w, int stream) {
    return ga_attn_grad(c, b, args, flags, w, stream, 0, "hnh_attn_grad_row_csr_p");
}
int hnh_attn_grad_col_csr_p(hnh_ctx* c, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* w, int stream) {
    return ga_attn_grad(c, b, args, flags, w, stream, 1, "hnh_attn_grad_col_csr_p");
}

int hnh_attn_grad_pack_f64(hnh_ctx* c, double* P, int64_t ld_p, const double* A, int64_t ld_a, const double* dZ, int64_t ld_dz, const double* lse,
                           const double* delta, int64_t rows, int f, int stream) {
    const char* who = "hnh_attn_grad_pack_f64";
    if (rows < 0) return ga_fail(c, HNH_ERR_INVALID, who, "negative size");
    if (f <= 0) return ga_fail(c, HNH_ERR_INVALID, who, "R must be positive");
    if ((lse == NULL) != (delta == NULL)) return ga_fail(c, HNH_ERR_INVALID, who, "lse and delta go together");
    const int fp = f + (f & 1), pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, lse != NULL);
    if (ld_p < pw || ld_p % 2 != 0 || ld_a < f || ld_dz < f) return ga_fail(c, HNH_ERR_INVALID, who, "bad pitch");
    if (rows == 0) return HNH_OK;
    if (!P || !A || !dZ) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_attn_grad_pack_f64");
    GA_R(A, ld_a, rows, f);
    GA_R(dZ, ld_dz, rows, f);
    if (lse) {
        GA_R(lse, rows, 1, rows);
        GA_R(delta, rows, 1, rows);
    }
    GA_W(P, ld_p, rows, pw);
    GA_PERFORM(c, who);
    for (int64_t r = 0; r < rows; r++) {
        double* p = P + r * ld_p;
        for (int k = 0; k < pw; k++) p[k] = 0.0;
        for (int k = 0; k < f; k++) {
            p[k] = A[r * ld_a + k];
            p[fp + k] = dZ[r * ld_dz + k];
        }
        if (lse) {
            p[2 * fp] = lse[r];
            p[2 * fp + 1] = delta[r];
        }
    }
    return HNH_OK;
}

/* ------------------------------------------------------------------------------------------------ include/hnh_train.h */
int64_t hnh_xent_rows_f64_workspace(int64_t rows) { return 3 * (rows < 1 ? 1 : (rows > 4096 ? 4096 : rows)); }  /* three partials per workgroup, at most 4096 */

int hnh_xent_rows_f64(hnh_ctx* c, const double* out, int64_t ld_out, const int32_t* labels, int64_t rows, int heads, int classes, double inv_n,
                      double* G, int64_t ld_g, double* result, double* work, int64_t work_doubles, int stream) {
    const char* who = "hnh_xent_rows_f64";
    if (rows < 0 || heads < 1 || classes < 1) return ga_fail(c, HNH_ERR_INVALID, who, "bad shape");
    if ((int64_t)heads * classes > HNH_XENT_MAX_WIDTH) return ga_fail(c, HNH_ERR_INVALID, who, "rows of heads * classes doubles exceed HNH_XENT_MAX_WIDTH");
    const int n = heads * classes;
    if (ld_out < n || (G && ld_g < n)) return ga_fail(c, HNH_ERR_INVALID, who, "bad pitch");
    if (!result || !work || work_doubles < hnh_xent_rows_f64_workspace(rows)) return ga_fail(c, HNH_ERR_INVALID, who, "null result or short workspace");
    if (rows > 0 && (!out || !labels)) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    HB_OP(c, stream, "hnh_xent_rows_f64");
    GA_R(out, ld_out, rows, n);
    if (rows > 0) HB_R(labels, (size_t)rows * sizeof(int32_t));
    if (G) GA_W(G, ld_g, rows, n);
    HB_W(work, (size_t)hnh_xent_rows_f64_workspace(rows) * sizeof(double));
    HB_W(result, 2 * sizeof(double));
    GA_PERFORM(c, who);
    double* z = (double*)malloc(sizeof(double) * (size_t)classes);
    if (!z) return ga_fail(c, HNH_ERR_NOMEM, who, "malloc failed");
    double loss = 0.0, correct = 0.0, bad = 0.0;
    for (int64_t r = 0; r < rows; r++) {
        int label = labels[r];
        if (label >= classes) {  /* reported in the results, never read out of range */
            bad += 1.0;
            label = -1;
        }
        if (label < 0) {
            if (G)
                for (int j = 0; j < n; j++) G[r * ld_g + j] = 0.0;
            continue;
        }
        int arg = 0;
        for (int k = 0; k < classes; k++) {
            double s = 0.0;
            for (int h = 0; h < heads; h++) s += out[r * ld_out + h * classes + k];
            z[k] = heads > 1 ? s * (1.0 / (double)heads) : s;
            if (z[k] > z[arg]) arg = k;  /* a tie keeps the lowest index */
        }
        const double mx = z[arg], zl = z[label];
        double sum = 0.0;
        for (int k = 0; k < classes; k++) {
            z[k] = exp(z[k] - mx);
            sum += z[k];
        }
        loss -= (zl - mx) - log(sum);
        correct += arg == label ? 1.0 : 0.0;
        if (G) {
            const double scale = inv_n * (1.0 / (double)heads);
            for (int j = 0; j < n; j++) G[r * ld_g + j] = scale * (z[j % classes] / sum - (j % classes == label ? 1.0 : 0.0));
        }
    }
    free(z);
    work[0] = loss; work[1] = correct; work[2] = bad;  /* one "workgroup" */
    result[0] = bad > 0.0 ? NAN : loss;
    result[1] = bad > 0.0 ? -bad : correct;
    return HNH_OK;
}

int hnh_optim_step_f64(hnh_ctx* c, const hnh_optim_tensor* tensors, int n, const hnh_optim* hy, int stream) {
    const char* who = "hnh_optim_step_f64";
    if (n < 0 || (n > 0 && !tensors) || !hy) return ga_fail(c, HNH_ERR_INVALID, who, "null table or negative count");
    if (hy->kind != HNH_OPTIM_ADAM && hy->kind != HNH_OPTIM_SGD) return ga_fail(c, HNH_ERR_INVALID, who, "unknown optimizer kind");
    const int adam = hy->kind == HNH_OPTIM_ADAM;
    if (adam && !(hy->bias1 > 0.0 && hy->bias2 > 0.0)) return ga_fail(c, HNH_ERR_INVALID, who, "Adam's bias corrections must be positive");
    for (int k = 0; k < n; k++) {
        const hnh_optim_tensor* t = &tensors[k];
        if (t->rows < 0 || t->cols < 0 || t->ld_p < t->cols || t->ld_g < t->cols) return ga_fail(c, HNH_ERR_INVALID, who, "bad shape or pitch");
        if (t->rows * t->cols > 0 && (!t->p || !t->g || !t->v || (adam && !t->m))) return ga_fail(c, HNH_ERR_INVALID, who, "null pointer");
    }
    HB_OP(c, stream, "hnh_optim_step_f64");
    for (int k = 0; k < n; k++) {
        const hnh_optim_tensor* t = &tensors[k];
        const int64_t total = t->rows * t->cols;
        if (total == 0) continue;
        GA_R(t->g, t->ld_g, t->rows, t->cols);
        GA_OUT(t->p, t->ld_p, t->rows, t->cols, 0);
        GA_OUT(t->v, total, 1, total, 0);
        if (adam) GA_OUT(t->m, total, 1, total, 0);
    }
    GA_PERFORM(c, who);
    for (int k = 0; k < n; k++) {
        const hnh_optim_tensor* t = &tensors[k];
        const int64_t total = t->rows * t->cols;
        for (int64_t i = 0; i < total; i++) {
            const int64_t r = i / t->cols, j = i % t->cols;
            double* pp = t->p + r * t->ld_p + j;
            const double p = *pp, gd = t->g[r * t->ld_g + j] + hy->weight_decay * p;
            if (adam) {
                const double m = hy->beta1 * t->m[i] + (1.0 - hy->beta1) * gd, v = hy->beta2 * t->v[i] + (1.0 - hy->beta2) * gd * gd;
                t->m[i] = m;
                t->v[i] = v;
                *pp = p - hy->lr * (m / hy->bias1) / (sqrt(v / hy->bias2) + hy->eps);
            } else {
                const double v = hy->momentum * t->v[i] + gd;
                t->v[i] = v;
                *pp = p - hy->lr * v;
            }
        }
    }
    return HNH_OK;
}
