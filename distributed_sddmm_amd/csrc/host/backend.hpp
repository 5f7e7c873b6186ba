// Function table over the C ABI of include/hnh_kernels.h.  The host layer never links the HIP library:
// it dlopen()s it (default: libhnh_kernels.so next to this library) and fails loudly if that is not
// possible.  There is NO built-in CPU implementation; the only other implementation of this ABI in the
// repository is the test double under oracle/ (built twice: with and without four of the optional groups), which tests load
// explicitly by path.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "hnh_attention.h"
#include "hnh_attn_additive.h"
#include "hnh_attn_dropout.h"
#include "hnh_attn_grad.h"
#include "hnh_attn_coef.h"
#include "hnh_attn_v2.h"
#include "hnh_attn_qkv.h"
#include "hnh_attn_edge.h"
#include "hnh_attn_edge_grad.h"
#include "hnh_gat_skip.h"
#include "hnh_gat_norm.h"
#include "hnh_grad.h"
#include "hnh_kernels.h"
#include "hnh_train.h"
#include "hnh_train_clip.h"
#include "hnh_train_multilabel.h"
#include "hnh_als_implicit.h"
#include "hnh_topk.h"
#include "hnh_rank.h"
#ifdef HNH_MEASUREMENT_AIDS
#include "hnh_measurement_aids.h"
#endif

// The kernels of the C ABI, each named ONCE: the members of Backend, their binding in load_backend() and the symbol -> header lookup of
// Backend::missing_kernel() are all generated from these two lists.
// MANDATORY, one group per line in the members' order (which drivers compiled earlier rely on): load_backend() fails when the library lacks one.
#define HNH_MANDATORY_KERNELS(X) \
    X(hnh_backend_name) X(hnh_ctx_create) X(hnh_ctx_destroy) X(hnh_last_error) X(hnh_ctx_stream) X(hnh_ctx_device_identity) /* the library and its contexts */ \
    X(hnh_malloc) X(hnh_free) X(hnh_memcpy) X(hnh_memset) X(hnh_stream_sync) /* memory and streams */ \
    X(hnh_event_create) X(hnh_event_destroy) X(hnh_event_record) X(hnh_event_wait) X(hnh_event_sync) X(hnh_event_query) X(hnh_event_elapsed_ms) /* events */ \
    X(hnh_sddmm_coo) X(hnh_sddmm_csr) X(hnh_spmm_csr) X(hnh_fused_sddmm_spmm_csr) X(hnh_sddmm_csr_ex) X(hnh_spmm_csr_ex) X(hnh_fused_sddmm_spmm_csr_ex) X(hnh_csr_max_row_nnz) /* SDDMM, SpMM and the fused pair */ \
    X(hnh_fused_sddmm_spmm_csr_x) X(hnh_row_epilogue_f64) X(hnh_row_epilogue_x) X(hnh_cg_step_f64) /* row epilogue and CG */ \
    X(hnh_tuples_sort) X(hnh_tuples_bucket_starts) X(hnh_tuples_transform) X(hnh_tuples_to_csr) /* tuples to CSR */ \
    X(hnh_csr_window_bounds) X(hnh_sddmm_csr_w) X(hnh_spmm_csr_w) X(hnh_fused_sddmm_spmm_csr_w) X(hnh_tuples_remap_cols) X(hnh_tuples_dedup_max) X(hnh_tuples_take_strided) /* row windows; tuple clean-up */ \
    X(hnh_panel_count) X(hnh_generate_er_keys) X(hnh_generate_rmat_keys) X(hnh_tuples_from_keys) X(hnh_tuples_relabel) /* panels; generators */ \
    X(hnh_fill_f64) X(hnh_hadamard_f64) X(hnh_axpy_f64) X(hnh_expand_rowptr) X(hnh_sum_chunked_blocks_f64) X(hnh_rowdot_f64) X(hnh_row_scale_add_f64) X(hnh_vec_add_scalar_f64) X(hnh_vec_div_f64) X(hnh_fill_hashed_f64) /* vectors, rows and scalars */ \
    X(hnh_gemm_f64) X(hnh_leaky_relu_f64) X(hnh_relu_store_cols_f64) /* dense */ \
    X(hnh_comm_unique_id) X(hnh_comm_init) X(hnh_comm_split) X(hnh_comm_destroy) X(hnh_comm_identity) /* communicators */ \
    X(hnh_comm_sendrecv) X(hnh_comm_group_begin) X(hnh_comm_group_end) X(hnh_comm_allgather) X(hnh_comm_reduce_scatter_f64) X(hnh_comm_allreduce_f64) /* collectives */ \
    X(hnh_ipc_export) X(hnh_ipc_open) X(hnh_ipc_close) X(hnh_ipc_pull) X(hnh_ipc_flags_register) X(hnh_ipc_flags_unregister) X(hnh_stream_write_flag) X(hnh_stream_wait_flag) /* ipc and stream flags */ \
    X(hnh_csr_plan_create) X(hnh_csr_plan_destroy) X(hnh_sddmm_csr_p) X(hnh_sddmm_csr_ps) X(hnh_spmm_csr_p) X(hnh_spmm_csr_pf) X(hnh_fused_sddmm_spmm_csr_p) /* planned row kernels */
// OPTIONAL, X(header, symbol): bound when the library exports it, null otherwise (of the two CPU test doubles only
// oracle/liboracle_backend_gat.so has the groups of hnh_grad.h, hnh_attention.h, hnh_attn_grad.h and hnh_train.h); whoever needs one refuses with
// Backend::missing_kernel(), which names the symbol and the header of its group:
//   hnh_grad.h: GAT::backwardPass; hnh_act_grad_cols_f64's presence also says that the library knows the HNH_ATTN_ACT_* flags (a non-ReLU layer)
//   hnh_attention.h: the GAT's softmax attention
//   hnh_attn_grad.h: the GAT's fused backward mode
//   hnh_attn_additive.h: the GAT's additive score
//   hnh_attn_dropout.h: the GAT's dropout
//   hnh_train.h: the GAT's loss, optimizer and training step
//   hnh_attn_v2.h: the GAT's gatv2 score
//   hnh_attn_qkv.h: the GAT's transformer score
//   hnh_attn_edge.h: a GAT layer with an edge bias
//   hnh_attn_edge_grad.h: a GAT layer whose edge bias is learned
//   hnh_attn_coef.h: GAT::attention_coefficients
//   hnh_gat_skip.h: a GAT layer with a bias or a skip connection (its presence also says that the library knows the HNH_ATTN_ADDEND flag)
//   hnh_gat_norm.h: a normalised GAT layer
//   hnh_train_multilabel.h: the GAT's multi-label (sigmoid) head
//   hnh_train_clip.h: the GAT's gradient clipping and its AdamW optimizer
//   hnh_als_implicit.h: Implicit_ALS in folded mode
//   hnh_topk.h: Implicit_ALS::recommend
//   hnh_rank.h: Implicit_ALS::rank_of
#define HNH_OPTIONAL_KERNELS(X) \
    X("include/hnh_grad.h", hnh_gemm_tn_f64_workspace) X("include/hnh_grad.h", hnh_gemm_tn_f64) X("include/hnh_grad.h", hnh_leaky_relu_grad_f64) X("include/hnh_grad.h", hnh_relu_grad_cols_f64) \
    X("include/hnh_grad.h", hnh_sum3_cols_f64) X("include/hnh_grad.h", hnh_transpose_into_f64) X("include/hnh_grad.h", hnh_act_grad_cols_f64) \
    X("include/hnh_attention.h", hnh_attn_softmax_csr_p) X("include/hnh_attention.h", hnh_softmax_gate_f64) X("include/hnh_attention.h", hnh_rowdot_cols_f64) \
    X("include/hnh_attn_grad.h", hnh_attn_grad_row_csr_p) X("include/hnh_attn_grad.h", hnh_attn_grad_col_csr_p) X("include/hnh_attn_grad.h", hnh_attn_grad_pack_f64) \
    X("include/hnh_attn_additive.h", hnh_attn_add_fwd_csr_p) X("include/hnh_attn_additive.h", hnh_attn_add_row_csr_p) X("include/hnh_attn_additive.h", hnh_attn_add_col_csr_p) \
    X("include/hnh_attn_additive.h", hnh_attn_add_scores_f64) X("include/hnh_attn_additive.h", hnh_attn_add_pack_f64) X("include/hnh_attn_additive.h", hnh_attn_add_update_f64) \
    X("include/hnh_attn_dropout.h", hnh_attn_drop_fwd_csr_p) X("include/hnh_attn_dropout.h", hnh_attn_drop_row_csr_p) X("include/hnh_attn_dropout.h", hnh_attn_drop_col_csr_p) \
    X("include/hnh_attn_dropout.h", hnh_attn_drop_scores_f64) X("include/hnh_attn_dropout.h", hnh_attn_drop_pack_f64) X("include/hnh_attn_dropout.h", hnh_feat_drop_f64) X("include/hnh_attn_dropout.h", hnh_dropout_words_u32) \
    X("include/hnh_train.h", hnh_xent_rows_f64_workspace) X("include/hnh_train.h", hnh_xent_rows_f64) X("include/hnh_train.h", hnh_optim_step_f64) \
    X("include/hnh_attn_v2.h", hnh_attn_v2_fwd_csr_p) X("include/hnh_attn_v2.h", hnh_attn_v2_row_csr_p) X("include/hnh_attn_v2.h", hnh_attn_v2_col_csr_p) X("include/hnh_attn_v2.h", hnh_attn_v2_finish_f64) \
    X("include/hnh_attn_qkv.h", hnh_attn_qkv_fwd_csr_p) X("include/hnh_attn_qkv.h", hnh_attn_qkv_row_csr_p) X("include/hnh_attn_qkv.h", hnh_attn_qkv_col_csr_p) \
    X("include/hnh_attn_edge.h", hnh_attn_qkv_bias_fwd_csr_p) X("include/hnh_attn_edge.h", hnh_attn_qkv_bias_row_csr_p) X("include/hnh_attn_edge.h", hnh_attn_qkv_bias_col_csr_p) \
    X("include/hnh_attn_edge_grad.h", hnh_attn_qkv_bias_grad_row_csr_p) X("include/hnh_attn_edge_grad.h", hnh_attn_qkv_bias_grad_col_csr_p) \
    X("include/hnh_attn_coef.h", hnh_attn_coef_csr_p) X("include/hnh_attn_coef.h", hnh_attn_coef_scores_f64) \
    X("include/hnh_gat_skip.h", hnh_skip_addend_cols_f64) X("include/hnh_gat_skip.h", hnh_skip_grad_cols_f64) X("include/hnh_gat_skip.h", hnh_colsum_f64_workspace) X("include/hnh_gat_skip.h", hnh_colsum_f64) \
    X("include/hnh_gat_norm.h", hnh_layernorm_fwd_f64) X("include/hnh_gat_norm.h", hnh_layernorm_bwd_workspace) X("include/hnh_gat_norm.h", hnh_layernorm_bwd_f64) \
    X("include/hnh_train_multilabel.h", hnh_bce_rows_f64_workspace) X("include/hnh_train_multilabel.h", hnh_bce_rows_f64) \
    X("include/hnh_train_clip.h", hnh_grad_sumsq_f64_workspace) X("include/hnh_train_clip.h", hnh_grad_sumsq_f64) X("include/hnh_train_clip.h", hnh_optim_step_clip_f64) \
    X("include/hnh_als_implicit.h", hnh_gram_rows_f64) \
    X("include/hnh_topk.h", hnh_topk_rows_f64_workspace) X("include/hnh_topk.h", hnh_topk_rows_f64) X("include/hnh_topk.h", hnh_topk_merge_f64) X("include/hnh_topk.h", hnh_take_rows_f64) \
    X("include/hnh_rank.h", hnh_pair_scores_f64) X("include/hnh_rank.h", hnh_rank_rows_f64_workspace) X("include/hnh_rank.h", hnh_rank_rows_f64) X("include/hnh_rank.h", hnh_rank_exclude_f64)

namespace hnh {

struct Backend {
    void* dl = nullptr;
    std::string path, name;

#define HNH_FN(sym) decltype(&::sym) sym = nullptr;
#define HNH_FN_OPTIONAL(header, sym) HNH_FN(sym)
    HNH_MANDATORY_KERNELS(HNH_FN)
    HNH_OPTIONAL_KERNELS(HNH_FN_OPTIONAL)
#ifdef HNH_MEASUREMENT_AIDS
    HNH_FN(hnh_stream_delay_us) HNH_FN(hnh_stream_paced_copy) HNH_FN(hnh_stream_pace_begin) HNH_FN(hnh_stream_pace_end)
#endif
#undef HNH_FN_OPTIONAL
#undef HNH_FN
    // "Error, <who> needs the kernel <symbol>, which the kernel library <path> does not export (<header>)": the one refusal of an optional
    // kernel that the library lacks; the header is the symbol's in HNH_OPTIONAL_KERNELS
    std::string missing_kernel(const std::string& who, const char* symbol) const;
};

// Loads (once per path) and returns the backend; path == nullptr or "" selects the product HIP library.
// Calls hnh::fatal() (print + exit(1) / exception) if the library or any mandatory symbol is missing.
Backend* load_backend(const char* path);
Backend* default_backend();           // the most recently loaded one; loads the HIP library on first use
std::string default_backend_path();   // <dir of libhnh_host.so>/libhnh_kernels.so

}  // namespace hnh
