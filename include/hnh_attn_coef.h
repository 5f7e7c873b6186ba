/*
 * hnh_attn_coef.h — export of the GAT's per-edge attention coefficients (GAT::attention_coefficients, csrc/host/gat.hpp) in every score
 * mode, exported by libhnh_kernels.so.
 *
 * An OPTIONAL group of the kernel ABI, like include/hnh_attn_v2.h: the host layer binds it with dlsym and leaves it null when a kernel
 * library does not export it (neither CPU test double under oracle/ does); the export then fails with an error naming the missing
 * symbol, and nothing else needs it.  Conventions as in hnh_kernels.h: device pointers, row-major fp64, int status, asynchronous.
 *
 * Per head, with A = X W_h (rows x f), alpha the LeakyReLU slope and lse_i the log-sum-exp that a finished forward pass stored, for every
 * nonzero e = (i, j) of the call (a repeated pair counts as often as it appears):
 *     values[e] = exp(z_e - lse_i)
 *     HNH_ATTN_COEF_DOT       z = LeakyReLU(<A_i, A_j>)                     (include/hnh_attention.h)
 *     HNH_ATTN_COEF_ADDITIVE  z = LeakyReLU(s_i + t_j), s = A a1, t = A a2  (include/hnh_attn_additive.h)
 *     HNH_ATTN_COEF_GATV2     z = sum_c a_c LeakyReLU(A_ic + A_jc)          (include/hnh_attn_v2.h)
 * One pass over the nonzeros, no reduction across a row: a value depends on its own operands alone, so results are bit-identical for any
 * split of a row into windows, groups of windows or Infinity-Cache panels, and run to run.  No atomics.
 *
 * DOT and GATV2 gather A_j (f doubles per nonzero), with A_i (and a) in registers: the layout of the forward passes.  ADDITIVE needs two
 * scalars per gathered row, not the row: its gathered operand is the PACKED PAIR
 *     T_r = [ t_r | id_r ]          HNH_ATTN_COEF_PAIR_WIDTH = 2 doubles, a 16-byte aligned base and an even pitch
 * (id_r = the row's global id as a double, exact below 2^53: it travels in the operand as in include/hnh_attn_dropout.h), 16 bytes per
 * nonzero instead of the fp + 4 doubles of the scored operand M'; s_i is read per row from args->s.  hnh_attn_coef_scores_f64 builds s and
 * T from A in one read, with the summation order of hnh_attn_add_scores_f64 (so s and t have the forward pass's bits).  (The alternative,
 * hnh_attn_add_scores_f64 and a strided view of M's last columns, would gather 16 bytes out of rows (fp + 2) doubles apart and move whole
 * rows of M between ranks; the pair is what a schedule moves here.)
 *
 * With `drop` (ADDITIVE only, as in the forward pass): values[e] = scale m_e exp(z_e - lse_i), the mask of include/hnh_attn_dropout.h —
 * the same key (seed, w2, global row, global column), the same integer keep test, so every copy of a repeated pair gets the same mask.
 * The own row's id is drop->row_id0 + the local row; the gathered row's id is T's second column.
 *
 * Widths: every f <= HNH_ATTN_COEF_MAX_F; 64, 128 and 256 run exact-width instances (16-byte aligned operands with even pitches), every
 * other width a bounds-checked one (8-byte lanes when f is odd or an operand is misaligned): the rules of hnh_attn_grad.h.  A wider head
 * returns HNH_ERR_UNSUPPORTED and writes nothing.  (ADDITIVE does not depend on f beyond that check.)
 */
#ifndef HNH_ATTN_COEF_H
#define HNH_ATTN_COEF_H
#include "hnh_attn_dropout.h" /* hnh_attn_drop */
#include "hnh_kernels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HNH_ATTN_COEF_MAX_F 256
#define HNH_ATTN_COEF_PAIR_WIDTH 2
#define HNH_ATTN_COEF_DOT 0
#define HNH_ATTN_COEF_ADDITIVE 1
#define HNH_ATTN_COEF_GATV2 2

typedef struct hnh_attn_coef {   /* 72 bytes */
    const double* X;    /* DOT, GATV2: the block's OWN rows of A (ld_x >= f) */
    int64_t ld_x;
    const double* a;    /* GATV2: the head's vector, f entries */
    const double* s;    /* ADDITIVE: s_i of the block's own rows, one per row */
    const double* lse;  /* lse_i of the block's own rows: the final values of the stored forward pass */
    const double* Y;    /* the gathered operand: A of the block's columns (DOT, GATV2; ld_y >= f) or the packed pair T (ADDITIVE; ld_y even, >= 2) */
    int64_t ld_y;
    int f;              /* head width */
    int score;          /* HNH_ATTN_COEF_DOT | _ADDITIVE | _GATV2 */
    double leaky_alpha;
} hnh_attn_coef;

/* One pass over a block of S, or over the selected window(s) of it: values[e] as above for every nonzero e of the call.  `values` is
 * addressed as hnh_sddmm_csr_ps addresses it (entry e of the block's CSR order, through windows, plans and panels; it may be a lent
 * slice of a caller's vector).  Every nonzero of the call is stored exactly once, nothing is read from `values`, nothing outside the
 * call's nonzeros is written.  Hub rows are walked by one group like every other row (a row has no state: nothing would be gained from
 * a second launch for them at the graph sizes a wave covers).  flags: 0.  drop != NULL needs score ADDITIVE (HNH_ERR_UNSUPPORTED
 * otherwise) and row ids below 2^32.  b->rowptr == NULL: no nonzeros, a no-op returning HNH_OK. */
int hnh_attn_coef_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, double* values, const hnh_attn_coef* args, const hnh_attn_drop* drop_or_null,
                        unsigned flags, const hnh_csr_window* window, int stream);

/* s[r] = <A_r, a1>,  T[r, :] = [<A_r, a2> | row_id0 + r] for r < rows: one read of A, one wave per row.  ld_t even and >= 2, T 16-byte
 * aligned; ld_a >= f; s and T must not alias A. */
int hnh_attn_coef_scores_f64(hnh_ctx* ctx, double* s, double* T, int64_t ld_t, const double* A, int64_t ld_a, const double* a1, const double* a2,
                             int64_t rows, int f, int64_t row_id0, int stream);

#ifdef __cplusplus
}
#endif
#endif /* HNH_ATTN_COEF_H */
