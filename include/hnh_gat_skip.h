/*
 * hnh_gat_skip.h — bias and skip (residual) connections of the GAT layers (GAT::set_bias / set_residual, csrc/host/gat.hpp), exported by
 * libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_grad.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); a layer with a bias or a residual then fails with an error
 * naming the missing symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status,
 * asynchronous.
 *
 * A layer's output is out[:, block h] = phi(o_h + r[:, block h] + b[block h]): the head's attention aggregate o_h, the residual r (the
 * layer input or its projection) and the bias b meet BEFORE the activation.  The addend r + b of a head is written into the head's
 * column block of the layer output (hnh_skip_addend_cols_f64), and the finishing call of the head's attention pass reads it there and
 * overwrites it with the activated sum (HNH_ATTN_ADDEND): the argument structs of the passes keep their sizes.  The backward pass stores
 * neither the pre-activation nor the addend: hnh_skip_grad_cols_f64 recovers o from the stored output and the recomputed addend.
 */
#ifndef HNH_GAT_SKIP_H
#define HNH_GAT_SKIP_H
#include "hnh_attention.h"
#include "hnh_grad.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Flag of the four forward attention entry points (hnh_attn_softmax_csr_p, hnh_attn_add_fwd_csr_p, hnh_attn_drop_fwd_csr_p,
 * hnh_attn_v2_fwd_csr_p), meaningful only together with HNH_ATTN_FINISH (without it: HNH_ERR_INVALID, nothing written): the finishing
 * call READS relu_dst[i * relu_ld + c] as the addend and writes act(o_i[c] + addend) to the same place, act being the ReLU or what an
 * HNH_ATTN_ACT_* flag names.  A row without nonzeros writes act(addend).  Every element is read and then written by the same lane.
 * lse and the row state do not depend on the flag, and a call without it computes what it computed before the flag existed, bit for
 * bit.  A library that exports hnh_skip_grad_cols_f64 knows the flag. */
#define HNH_ATTN_ADDEND 0x40u

/* dst[r, col0 + c] = (res ? res[r * ld_res + c] : 0) + (bias ? bias[c] : 0) for r < rows, c < cols: one head's addend into the head's
 * column block of the layer output.  16-byte accesses when cols, col0, ld_dst (and ld_res) are even and dst (res, bias) 16-byte
 * aligned.  res must not overlap the written block. */
int hnh_skip_addend_cols_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t col0, const double* res, int64_t ld_res, const double* bias,
                             int64_t rows, int64_t cols, int stream);

/* hnh_act_grad_cols_f64 (hnh_grad.h) for a head whose pre-activation was o + addend, addend[r, c] = (res ? res[r * ld_res + c] : 0) +
 * (bias ? bias[c] : 0): dZ and delta of the head from G, the STORED output and the addend, in one pass over the column block
 * [col0, col0 + cols) of G and out.
 *     dZ       bit for bit hnh_act_grad_cols_f64's (it depends on G and out only), to dZ[r * ld_dz + c] and, when dZ_all is not null,
 *              also to dZ_all[r * ld_all + col0 + c]: every head's dZ in one rows x (H f) matrix for the bias and residual gradients
 *     delta_r  = sum_c dZ[r, c] * ((phi^{-1}(out[r, col0 + c]) - res[r, c]) - bias[c]), with phi^{-1}(out) = out for HNH_ACT_RELU (where
 *              out > 0; elsewhere dZ = 0 and the term is 0) and HNH_ACT_IDENTITY, and for HNH_ACT_ELU out where out >= 0 and log1p(out)
 *              below (the term is 0 where 1 + out == 0)
 * A power-of-two group of lanes owns a row; delta is summed in a fixed order (no atomics): bit-identical run to run.  16-byte accesses
 * when cols, col0 and every pitch in use are even and every base in use 16-byte aligned. */
int hnh_skip_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, double* dZ_all, int64_t ld_all, double* delta, const double* G, int64_t ld_g,
                           const double* out, int64_t ld_out, int64_t col0, const double* res, int64_t ld_res, const double* bias, int64_t rows,
                           int64_t cols, int act, int stream);

/* out[c] = sum over r < rows of src[r * ld + c], c < cols (the bias gradient).  Workgroups write the sums of consecutive row ranges
 * into `work` (each in a fixed order) and a second launch adds the ranges front to back: no atomics, bit-identical run to run; the
 * split depends on (rows, cols) only.  `work` must hold hnh_colsum_f64_workspace(rows, cols) doubles.  rows == 0 writes zeros. */
int64_t hnh_colsum_f64_workspace(int64_t rows, int64_t cols);
int hnh_colsum_f64(hnh_ctx* ctx, double* out, const double* src, int64_t ld, int64_t rows, int64_t cols, double* work, int64_t work_doubles,
                   int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_GAT_SKIP_H */
