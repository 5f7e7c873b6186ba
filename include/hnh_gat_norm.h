/*
 * hnh_gat_norm.h — layer normalisation of the GAT layers (GAT::set_norm, csrc/host/gat.hpp), exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_gat_skip.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); a normalised layer then fails with an error naming the
 * missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status, asynchronous.
 *
 * A normalised layer's output is out = phi(gamma o xh + beta) with, per WHOLE output row z_r = o_r + r_r + b (all heads side by side,
 * C columns):
 *     mu_r   = mean_c z_rc
 *     var_r  = mean_c (z_rc - mu_r)^2      biased and TWO-PASS: the deviations are formed before they are squared
 *     rstd_r = 1 / sqrt(var_r + eps),  xh_rc = (z_rc - mu_r) rstd_r,  y_rc = gamma_c xh_rc + beta_c,  out_rc = phi(y_rc)
 * phi is HNH_ACT_RELU, HNH_ACT_ELU (y for y >= 0, expm1(y) below) or HNH_ACT_IDENTITY (include/hnh_grad.h).  The backward pass, with
 * G = dL/d(out):
 *     dY = G o phi'(y)        (relu: y > 0;  elu: y >= 0 ? 1 : exp(y);  identity: 1)
 *     dgamma_c = sum_r dY_rc xh_rc,  dbeta_c = sum_r dY_rc,  t = gamma o dY
 *     dz_rc = rstd_r (t_rc - mean_c t_r - xh_rc mean_c (t_r o xh_r))
 * Both kernels hold a row in registers between its reductions and its store: z (and G) are read once from HBM.  Every reduction runs
 * in a fixed order without atomics: results are bit-identical run to run.  Accesses are 16 bytes per lane when cols and every pitch in
 * use are even and every matrix base 16-byte aligned, 8 bytes otherwise (gamma, beta, stats, dgamma and dbeta need 8-byte alignment only).
 */
#ifndef HNH_GAT_NORM_H
#define HNH_GAT_NORM_H
#include "hnh_grad.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The widest row the two kernels take: a row lives in the registers of one wave (cols <= 512, or 256 with 8-byte accesses) or of one
 * 256-lane workgroup.  A wider row returns HNH_ERR_UNSUPPORTED and writes nothing. */
#define HNH_NORM_MAX_COLS 4096

/* out[r, c] = phi(gamma[c] * xh[r, c] + beta[c]) for r < rows, c < cols, and stats[2 r] = mu_r, stats[2 r + 1] = rstd_r.
 * eps > 0 and finite.  out == z with ld_out == ld_z (in place) is allowed: every element is read and then written by the same lane;
 * any other overlap of out, z and stats is HNH_ERR_INVALID.  rows == 0 or cols == 0 is a no-op. */
int hnh_layernorm_fwd_f64(hnh_ctx* ctx, double* out, int64_t ld_out, const double* z, int64_t ld_z, double* stats, const double* gamma,
                          const double* beta, int64_t rows, int64_t cols, double eps, int act, int stream);

/* dz, dgamma and dbeta from G, the pre-normalisation rows z and the forward call's stats; y is recomputed, not stored, and the two row
 * means come from one reduction.  Column sums: a workgroup owns a consecutive range of rows, its lanes own fixed columns and add their
 * rows in row order into registers, and the workgroup writes one partial row pair into `work`; a second launch adds the ranges front to
 * back.  The split depends on (rows, cols) only.  `work` must hold hnh_layernorm_bwd_workspace(rows, cols) doubles.  dz == G with
 * ld_dz == ld_g is allowed; any other overlap of an output with an operand or another output is HNH_ERR_INVALID.  rows == 0 writes
 * zeros to dgamma and dbeta; cols == 0 is a no-op. */
int64_t hnh_layernorm_bwd_workspace(int64_t rows, int64_t cols);
int hnh_layernorm_bwd_f64(hnh_ctx* ctx, double* dz, int64_t ld_dz, double* dgamma, double* dbeta, const double* G, int64_t ld_g, const double* z,
                          int64_t ld_z, const double* stats, const double* gamma, const double* beta, int64_t rows, int64_t cols, int act,
                          double* work, int64_t work_doubles, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_GAT_NORM_H */
