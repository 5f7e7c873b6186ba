/*
 * hnh_grad.h — dense kernels of the GAT backward pass (GAT::backwardPass in csrc/host/gat.hpp), exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI: the host layer binds it with dlsym and leaves it null when a kernel library does not export
 * it (the plain CPU test double, oracle/liboracle_backend.so, does not; the second one, oracle/liboracle_backend_gat.so, does), and GAT::backwardPass then fails with an error naming the missing symbol.  The
 * forward pass and every other operation never need it.  No counterpart in the reference (its gat.hpp:43-48 leaves the backward
 * pass as work in progress).  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status, asynchronous.
 */
#ifndef HNH_GRAD_H
#define HNH_GRAD_H
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

/* C[M x N] = A^T * B with A stored K x M (leading dimension lda >= M) and B stored K x N (ldb >= N), C with ldc >= N: the weight
 * gradient X^T * dA, a reduction over every local row (K) into a small output.  fp64 matrix cores, split over K into S slices; the
 * slices write partial tiles into `work` and a second launch sums them in slice order, so results are bit-identical run to run.
 * S depends on (M, N, K) only.  `work` must hold hnh_gemm_tn_f64_workspace(M, N, K) doubles (none when it returns 0: then `work`
 * may be null).  No atomics. */
int64_t hnh_gemm_tn_f64_workspace(int64_t M, int64_t N, int64_t K);
int hnh_gemm_tn_f64(hnh_ctx* ctx, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                    double* C, int64_t ldc, double* work, int64_t work_doubles, int stream);

/* In place over two value vectors of n entries: e -> a = LeakyReLU_alpha(e) and da -> de = da * (e > 0 ? 1 : alpha). */
int hnh_leaky_relu_grad_f64(hnh_ctx* ctx, double* e_to_a, double* da_to_de, double alpha, int64_t n, int stream);

/* dZ[r, c] = out[r, col0 + c] > 0 ? G[r, col0 + c] : 0 for r < rows, c < cols (ReLU' from the stored output). */
int hnh_relu_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, const double* G, int64_t ld_g, const double* out, int64_t ld_out,
                           int64_t col0, int64_t rows, int64_t cols, int stream);

/* dZ and delta of one head from G and the STORED output of the head's activation, in one pass over the column block [col0, col0 + cols)
 * of G and out (each read once): dZ (rows x cols, pitch ld_dz) and delta (rows).  With o the activation's input recovered from out:
 *     HNH_ACT_RELU      dZ = out > 0 ? G : 0                      delta_r = sum_c dZ[r, c] out[r, c]   (hnh_relu_grad_cols_f64's dZ, bit for bit)
 *     HNH_ACT_IDENTITY  dZ = G                                    delta_r = sum_c G[r, c] out[r, c]
 *     HNH_ACT_ELU       dZ = G where out >= 0, G (1 + out) below  delta_r = sum_c dZ[r, c] o[r, c], o = out where out >= 0 and log1p(out) below;
 *                       the term is 0 where 1 + out == 0 (a unit saturated at -1 has dZ = 0)
 * A power-of-two group of lanes owns a row; delta is summed in a fixed order (no atomics): bit-identical run to run.  16-byte accesses
 * when cols, col0 and the three pitches are even and the three bases 16-byte aligned.  Replaces hnh_relu_grad_cols_f64 followed by
 * hnh_rowdot_cols_f64 (hnh_attention.h).  A kernel library that exports this symbol also knows the HNH_ATTN_ACT_* flags of the forward
 * passes (hnh_attention.h). */
#define HNH_ACT_RELU 0
#define HNH_ACT_ELU 1
#define HNH_ACT_IDENTITY 2
int hnh_act_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, double* delta, const double* G, int64_t ld_g, const double* out,
                          int64_t ld_out, int64_t col0, int64_t rows, int64_t cols, int act, int stream);

/* dst[r, col0 + c] = (x[r, c] + y[r, c]) + z[r, c]; x, y, z are rows x cols with leading dimension cols. */
int hnh_sum3_cols_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t col0, const double* x, const double* y, const double* z,
                      int64_t rows, int64_t cols, int stream);

/* dst[row0 + c, r] = W[r, c] for W of rows x cols (leading dimension cols): W^T into rows [row0, row0 + cols) of dst. */
int hnh_transpose_into_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t row0, const double* W, int64_t rows, int64_t cols,
                           int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_GRAD_H */
