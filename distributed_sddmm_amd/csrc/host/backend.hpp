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
#include "hnh_train_multilabel.h"
#ifdef HNH_MEASUREMENT_AIDS
#include "hnh_measurement_aids.h"
#endif

namespace hnh {

struct Backend {
    void* dl = nullptr;
    std::string path, name;

#define HNH_FN(sym) decltype(&::sym) sym = nullptr;
    HNH_FN(hnh_backend_name)
    HNH_FN(hnh_ctx_create) HNH_FN(hnh_ctx_destroy) HNH_FN(hnh_last_error) HNH_FN(hnh_ctx_stream) HNH_FN(hnh_ctx_device_identity)
    HNH_FN(hnh_malloc) HNH_FN(hnh_free) HNH_FN(hnh_memcpy) HNH_FN(hnh_memset) HNH_FN(hnh_stream_sync)
    HNH_FN(hnh_event_create) HNH_FN(hnh_event_destroy) HNH_FN(hnh_event_record) HNH_FN(hnh_event_wait)
    HNH_FN(hnh_event_sync) HNH_FN(hnh_event_query) HNH_FN(hnh_event_elapsed_ms)
    HNH_FN(hnh_sddmm_coo) HNH_FN(hnh_sddmm_csr) HNH_FN(hnh_spmm_csr) HNH_FN(hnh_fused_sddmm_spmm_csr)
    HNH_FN(hnh_sddmm_csr_ex) HNH_FN(hnh_spmm_csr_ex) HNH_FN(hnh_fused_sddmm_spmm_csr_ex) HNH_FN(hnh_csr_max_row_nnz)
    HNH_FN(hnh_fused_sddmm_spmm_csr_x) HNH_FN(hnh_row_epilogue_f64) HNH_FN(hnh_row_epilogue_x) HNH_FN(hnh_cg_step_f64)
    HNH_FN(hnh_tuples_sort) HNH_FN(hnh_tuples_bucket_starts) HNH_FN(hnh_tuples_transform) HNH_FN(hnh_tuples_to_csr)
    HNH_FN(hnh_csr_window_bounds) HNH_FN(hnh_sddmm_csr_w) HNH_FN(hnh_spmm_csr_w) HNH_FN(hnh_fused_sddmm_spmm_csr_w) HNH_FN(hnh_tuples_remap_cols) HNH_FN(hnh_tuples_dedup_max) HNH_FN(hnh_tuples_take_strided)
    HNH_FN(hnh_panel_count) HNH_FN(hnh_generate_er_keys) HNH_FN(hnh_generate_rmat_keys) HNH_FN(hnh_tuples_from_keys) HNH_FN(hnh_tuples_relabel)
    HNH_FN(hnh_fill_f64) HNH_FN(hnh_hadamard_f64) HNH_FN(hnh_axpy_f64) HNH_FN(hnh_expand_rowptr) HNH_FN(hnh_sum_chunked_blocks_f64)
    HNH_FN(hnh_rowdot_f64) HNH_FN(hnh_row_scale_add_f64) HNH_FN(hnh_vec_add_scalar_f64) HNH_FN(hnh_vec_div_f64) HNH_FN(hnh_fill_hashed_f64)
    HNH_FN(hnh_gemm_f64) HNH_FN(hnh_leaky_relu_f64) HNH_FN(hnh_relu_store_cols_f64)
    HNH_FN(hnh_comm_unique_id) HNH_FN(hnh_comm_init) HNH_FN(hnh_comm_split) HNH_FN(hnh_comm_destroy) HNH_FN(hnh_comm_identity)
    HNH_FN(hnh_comm_sendrecv) HNH_FN(hnh_comm_group_begin) HNH_FN(hnh_comm_group_end) HNH_FN(hnh_comm_allgather) HNH_FN(hnh_comm_reduce_scatter_f64)
    HNH_FN(hnh_comm_allreduce_f64)
    HNH_FN(hnh_ipc_export) HNH_FN(hnh_ipc_open) HNH_FN(hnh_ipc_close) HNH_FN(hnh_ipc_pull) HNH_FN(hnh_ipc_flags_register) HNH_FN(hnh_ipc_flags_unregister)
    HNH_FN(hnh_stream_write_flag) HNH_FN(hnh_stream_wait_flag)
    HNH_FN(hnh_csr_plan_create) HNH_FN(hnh_csr_plan_destroy) HNH_FN(hnh_sddmm_csr_p) HNH_FN(hnh_sddmm_csr_ps) HNH_FN(hnh_spmm_csr_p) HNH_FN(hnh_spmm_csr_pf) HNH_FN(hnh_fused_sddmm_spmm_csr_p)
    // OPTIONAL group (include/hnh_grad.h): bound when the library exports it, null otherwise (the plain CPU test double does not, oracle/liboracle_backend_gat.so does:
    // that one has this group and those of hnh_attention.h, hnh_attn_grad.h and hnh_train.h);
    // only GAT::backwardPass needs it, and it fails with an error naming the missing symbol
    HNH_FN(hnh_gemm_tn_f64_workspace) HNH_FN(hnh_gemm_tn_f64) HNH_FN(hnh_leaky_relu_grad_f64) HNH_FN(hnh_relu_grad_cols_f64)
    HNH_FN(hnh_sum3_cols_f64) HNH_FN(hnh_transpose_into_f64)
    // (its presence also says that the library knows the HNH_ATTN_ACT_* flags: only a GAT layer with a non-ReLU activation needs it)
    HNH_FN(hnh_act_grad_cols_f64)
    // OPTIONAL group (include/hnh_attention.h), bound the same way: only the GAT's softmax attention needs it
    HNH_FN(hnh_attn_softmax_csr_p) HNH_FN(hnh_softmax_gate_f64) HNH_FN(hnh_rowdot_cols_f64)
    // OPTIONAL group (include/hnh_attn_grad.h), bound the same way: only the GAT's fused backward mode needs it
    HNH_FN(hnh_attn_grad_row_csr_p) HNH_FN(hnh_attn_grad_col_csr_p) HNH_FN(hnh_attn_grad_pack_f64)
    // OPTIONAL group (include/hnh_attn_additive.h), bound the same way: only the GAT's additive score needs it
    HNH_FN(hnh_attn_add_fwd_csr_p) HNH_FN(hnh_attn_add_row_csr_p) HNH_FN(hnh_attn_add_col_csr_p)
    HNH_FN(hnh_attn_add_scores_f64) HNH_FN(hnh_attn_add_pack_f64) HNH_FN(hnh_attn_add_update_f64)
    // OPTIONAL group (include/hnh_attn_dropout.h), bound the same way: only the GAT's dropout needs it
    HNH_FN(hnh_attn_drop_fwd_csr_p) HNH_FN(hnh_attn_drop_row_csr_p) HNH_FN(hnh_attn_drop_col_csr_p)
    HNH_FN(hnh_attn_drop_scores_f64) HNH_FN(hnh_attn_drop_pack_f64) HNH_FN(hnh_feat_drop_f64) HNH_FN(hnh_dropout_words_u32)
    // OPTIONAL group (include/hnh_train.h), bound the same way: only the GAT's loss, optimizer and training step need it
    HNH_FN(hnh_xent_rows_f64_workspace) HNH_FN(hnh_xent_rows_f64) HNH_FN(hnh_optim_step_f64)
    // OPTIONAL group (include/hnh_attn_v2.h), bound the same way: only the GAT's gatv2 score needs it
    HNH_FN(hnh_attn_v2_fwd_csr_p) HNH_FN(hnh_attn_v2_row_csr_p) HNH_FN(hnh_attn_v2_col_csr_p) HNH_FN(hnh_attn_v2_finish_f64)
    // OPTIONAL group (include/hnh_attn_qkv.h), bound the same way: only the GAT's transformer score needs it
    HNH_FN(hnh_attn_qkv_fwd_csr_p) HNH_FN(hnh_attn_qkv_row_csr_p) HNH_FN(hnh_attn_qkv_col_csr_p)
    // OPTIONAL group (include/hnh_attn_edge.h), bound the same way: only a GAT layer with an edge bias needs it
    HNH_FN(hnh_attn_qkv_bias_fwd_csr_p) HNH_FN(hnh_attn_qkv_bias_row_csr_p) HNH_FN(hnh_attn_qkv_bias_col_csr_p)
    // OPTIONAL group (include/hnh_attn_edge_grad.h), bound the same way: only a GAT layer whose edge bias is learned needs it
    HNH_FN(hnh_attn_qkv_bias_grad_row_csr_p) HNH_FN(hnh_attn_qkv_bias_grad_col_csr_p)
    // OPTIONAL group (include/hnh_attn_coef.h), bound the same way: only GAT::attention_coefficients needs it
    HNH_FN(hnh_attn_coef_csr_p) HNH_FN(hnh_attn_coef_scores_f64)
    // OPTIONAL group (include/hnh_gat_skip.h), bound the same way: only a GAT layer with a bias or a skip connection needs it
    // (its presence also says that the library knows the HNH_ATTN_ADDEND flag)
    HNH_FN(hnh_skip_addend_cols_f64) HNH_FN(hnh_skip_grad_cols_f64) HNH_FN(hnh_colsum_f64_workspace) HNH_FN(hnh_colsum_f64)
    // OPTIONAL group (include/hnh_gat_norm.h), bound the same way: only a normalised GAT layer needs it
    HNH_FN(hnh_layernorm_fwd_f64) HNH_FN(hnh_layernorm_bwd_workspace) HNH_FN(hnh_layernorm_bwd_f64)
    // OPTIONAL group (include/hnh_train_multilabel.h), bound the same way: only the GAT's multi-label (sigmoid) head needs it
    HNH_FN(hnh_bce_rows_f64_workspace) HNH_FN(hnh_bce_rows_f64)
#ifdef HNH_MEASUREMENT_AIDS
    HNH_FN(hnh_stream_delay_us) HNH_FN(hnh_stream_paced_copy) HNH_FN(hnh_stream_pace_begin) HNH_FN(hnh_stream_pace_end)
#endif
#undef HNH_FN
};

// Loads (once per path) and returns the backend; path == nullptr or "" selects the product HIP library.
// Calls hnh::fatal() (print + exit(1) / exception) if the library or any mandatory symbol is missing.
Backend* load_backend(const char* path);
Backend* default_backend();           // the most recently loaded one; loads the HIP library on first use
std::string default_backend_path();   // <dir of libhnh_host.so>/libhnh_kernels.so

}  // namespace hnh
