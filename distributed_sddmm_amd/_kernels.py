"""ctypes binding of include/hnh_kernels.h (lib/libhnh_kernels.so).  Fails loudly if the HIP library
is missing or no GPU is present — there is no fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HNH_KERNEL_LIB_DEV") or os.path.join(HERE, "lib", "libhnh_kernels.so")  # override: kernel tuning experiments only

OK = 0
STREAM_COMPUTE, STREAM_COMM, STREAM_AUX = 0, 1, 2
H2D, D2H, D2D = 0, 1, 2
FUSED_VALUES_OVERWRITE, FUSED_OUT_OVERWRITE, FUSED_LEAKY_RELU = 1, 2, 4
UNIQUE_ID_BYTES = 128

_vp, _i32, _i64, _dbl, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t

# name -> (restype, argtypes): every symbol include/hnh_kernels.h declares
SIGNATURES = {
    "hnh_backend_name": (C.c_char_p, []),
    "hnh_ctx_create": (_i32, [_i32, C.POINTER(_vp)]),
    "hnh_ctx_destroy": (_i32, [_vp]),
    "hnh_last_error": (C.c_char_p, [_vp]),
    "hnh_ctx_stream": (_vp, [_vp, _i32]),
    "hnh_ctx_device_identity": (_i32, [_vp, C.POINTER(_i32), C.c_char_p, _i32]),
    "hnh_malloc": (_i32, [_vp, _sz, C.POINTER(_vp)]),
    "hnh_free": (_i32, [_vp, _vp]),
    "hnh_memcpy": (_i32, [_vp, _vp, _vp, _sz, _i32, _i32]),
    "hnh_memset": (_i32, [_vp, _vp, _i32, _sz, _i32]),
    "hnh_stream_sync": (_i32, [_vp, _i32]),
    "hnh_event_create": (_i32, [_vp, C.POINTER(_vp)]),
    "hnh_event_destroy": (_i32, [_vp, _vp]),
    "hnh_event_record": (_i32, [_vp, _vp, _i32]),
    "hnh_event_wait": (_i32, [_vp, _vp, _i32]),
    "hnh_event_sync": (_i32, [_vp, _vp]),
    "hnh_event_query": (_i32, [_vp, _vp, _vp]),
    "hnh_event_elapsed_ms": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float)]),
    "hnh_sddmm_coo": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "hnh_sddmm_csr": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "hnh_spmm_csr": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "hnh_fused_sddmm_spmm_csr": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _i32]),
    "hnh_sddmm_csr_ex": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i64, _i32]),
    "hnh_spmm_csr_ex": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i64, _i32]),
    "hnh_fused_sddmm_spmm_csr_ex": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _i64, _i32, _i64, _i32]),
    "hnh_panel_count": (_i32, [_vp, _i64, _i64, _i64, _i32, _i32]),
    "hnh_csr_window_bounds": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32]),
    "hnh_sddmm_csr_w": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _i32]),
    "hnh_spmm_csr_w": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _i32]),
    "hnh_fused_sddmm_spmm_csr_w": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _i64, _i32, _vp, _vp, _i32]),
    "hnh_csr_max_row_nnz": (_i32, [_vp, _i64, _vp, C.POINTER(C.c_int), _i32]),
    "hnh_fused_sddmm_spmm_csr_x": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _i64, _i32, _i64, _vp, _i32]),
    "hnh_row_epilogue_f64": (_i32, [_vp, _vp, _vp, C.c_double, _vp, _i64, _i32, _i32]),
    "hnh_row_epilogue_x": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "hnh_cg_step_f64": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "hnh_tuples_sort": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32]),
    "hnh_tuples_bucket_starts": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i32]),
    "hnh_tuples_transform": (_i32, [_vp, _vp, _i64, _i32, C.c_uint64, C.c_uint64, _i32]),
    "hnh_tuples_remap_cols": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i32]),
    "hnh_tuples_dedup_max": (_i32, [_vp, _vp, _i64, C.POINTER(C.c_int64), _i32]),
    "hnh_tuples_take_strided": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i32]),
    "hnh_generate_er_keys": (_i32, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.POINTER(C.c_int64), _i32]),
    "hnh_generate_rmat_keys": (_i32, [_vp, _i32, C.c_uint64, _dbl, _dbl, _dbl, C.c_uint64, _i32, _vp, C.POINTER(C.c_int64), _i32]),
    "hnh_tuples_from_keys": (_i32, [_vp, _vp, C.c_uint64, _i64, _i64, C.c_double, _vp, _i64, _i32]),
    "hnh_tuples_relabel": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32]),
    "hnh_tuples_to_csr": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, C.POINTER(C.c_int), _i32]),
    "hnh_fill_f64": (_i32, [_vp, _vp, _i64, _dbl, _i32]),
    "hnh_hadamard_f64": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "hnh_axpy_f64": (_i32, [_vp, _vp, _vp, _dbl, _i64, _i32]),
    "hnh_expand_rowptr": (_i32, [_vp, _i64, _vp, _vp, _i32]),
    "hnh_rowdot_f64": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "hnh_row_scale_add_f64": (_i32, [_vp, _vp, _vp, _dbl, _vp, _vp, _dbl, _i64, _i32, _i32]),
    "hnh_vec_add_scalar_f64": (_i32, [_vp, _vp, _dbl, _i64, _i32]),
    "hnh_vec_div_f64": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "hnh_fill_hashed_f64": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, C.c_uint64, _dbl, _i32]),
    "hnh_gemm_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32]),
    "hnh_leaky_relu_f64": (_i32, [_vp, _vp, _dbl, _i64, _i32]),
    "hnh_relu_store_cols_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32]),
    "hnh_comm_unique_id": (_i32, [_vp]),
    "hnh_comm_init": (_i32, [_vp, _i32, _i32, _vp, C.POINTER(_vp)]),
    "hnh_comm_split": (_i32, [_vp, _vp, _i32, _i32, C.POINTER(_vp)]),
    "hnh_comm_destroy": (_i32, [_vp, _vp]),
    "hnh_comm_identity": (_i32, [_vp, _vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "hnh_comm_sendrecv": (_i32, [_vp, _vp, _vp, _sz, _i32, _vp, _sz, _i32, _i32]),
    "hnh_comm_group_begin": (_i32, [_vp]),
    "hnh_comm_group_end": (_i32, [_vp]),
    "hnh_comm_allgather": (_i32, [_vp, _vp, _vp, _vp, _sz, _i32]),
    "hnh_comm_reduce_scatter_f64": (_i32, [_vp, _vp, _vp, _vp, _sz, _i32]),
    "hnh_comm_allreduce_f64": (_i32, [_vp, _vp, _vp, _vp, _sz, _i32]),
    "hnh_ipc_export": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hnh_ipc_open": (_i32, [_vp, _vp, C.c_uint64, C.POINTER(_vp)]),
    "hnh_ipc_close": (_i32, [_vp, _vp]),
    "hnh_ipc_pull": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32]),
    "hnh_ipc_flags_register": (_i32, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "hnh_ipc_flags_unregister": (_i32, [_vp, _vp]),
    "hnh_stream_write_flag": (_i32, [_vp, _i32, _vp, C.c_uint64]),
    "hnh_stream_wait_flag": (_i32, [_vp, _i32, _vp, C.c_uint64]),
    "hnh_csr_plan_create": (_i32, [_vp, C.POINTER(_vp)]),
    "hnh_csr_plan_destroy": (_i32, [_vp, _vp]),
    "hnh_sddmm_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _i32]),
    "hnh_sddmm_csr_ps": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _i32]),
    "hnh_spmm_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32]),
    "hnh_sum_chunked_blocks_f64": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32]),
    "hnh_spmm_csr_pf": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _i32]),
    "hnh_fused_sddmm_spmm_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _vp, _i32]),
}


# include/hnh_measurement_aids.h (tools and their tests only)
AIDS_SIGNATURES = {
    "hnh_stream_delay_us": (_i32, [_vp, _i32, C.c_double]),
    "hnh_stream_paced_copy": (_i32, [_vp, _i32, _vp, _vp, C.c_size_t, _i32, C.c_double, _i32]),
    "hnh_stream_pace_begin": (_i32, [_vp, _i32]),
    "hnh_stream_pace_end": (_i32, [_vp, _i32, C.c_double]),
}


# include/hnh_grad.h: the dense kernels of the GAT backward pass, an OPTIONAL group bound only for the product library (the CPU test
# double under oracle/ does not export it; the host layer binds it with dlsym and reports the missing symbol when it is needed)
GRAD_SIGNATURES = {
    "hnh_gemm_tn_f64_workspace": (_i64, [_i64, _i64, _i64]),
    "hnh_gemm_tn_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32]),
    "hnh_leaky_relu_grad_f64": (_i32, [_vp, _vp, _vp, _dbl, _i64, _i32]),
    "hnh_relu_grad_cols_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32]),
    "hnh_act_grad_cols_f64": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32]),
    "hnh_sum3_cols_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32]),
    "hnh_transpose_into_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32]),
}


# include/hnh_attention.h: neighbourhood-softmax attention of the GAT, a second OPTIONAL group bound only for the product library (the
# CPU test double does not export it; the host layer binds it with dlsym and names the missing symbol when the softmax mode needs it)
ATTN_SIGNATURES = {
    "hnh_attn_softmax_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _vp, _i32]),
    "hnh_softmax_gate_f64": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _i64, _i32]),
    "hnh_rowdot_cols_f64": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32]),
}
ATTN_FINISH = 8  # HNH_ATTN_FINISH
ATTN_ACT_ELU, ATTN_ACT_IDENTITY = 0x10, 0x20  # HNH_ATTN_ACT_*: the finishing call's output activation (neither: ReLU)
ACT_RELU, ACT_ELU, ACT_IDENTITY = 0, 1, 2     # HNH_ACT_* of hnh_act_grad_cols_f64


# include/hnh_attn_grad.h: the fused backward pass of the GAT's attention, a third OPTIONAL group bound only for the product library
ATTN_GRAD_SIGNATURES = {
    "hnh_attn_grad_row_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_grad_col_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_grad_pack_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32]),
}
ATTN_GRAD_MAX_F = 256  # HNH_ATTN_GRAD_MAX_F
ERR_UNSUPPORTED = 4    # HNH_ERR_UNSUPPORTED


def attn_grad_packed_width(f: int, softmax: bool) -> int:
    """HNH_ATTN_GRAD_PACKED_WIDTH"""
    return 2 * (f + (f & 1)) + (2 if softmax else 0)


class AttnGrad(C.Structure):
    """struct hnh_attn_grad"""
    _fields_ = [("X", _vp), ("ld_x", _i64), ("dZ", _vp), ("ld_dz", _i64), ("lse", _vp), ("delta", _vp), ("Y", _vp), ("ld_y", _i64),
                ("Out", _vp), ("ld_out", _i64), ("f", _i32), ("softmax", _i32), ("leaky_alpha", _dbl)]


# include/hnh_attn_additive.h: additive (a1, a2) attention scores of the GAT, forward and backward; a fourth OPTIONAL group bound only
# for the product library
ATTN_ADD_SIGNATURES = {
    "hnh_attn_add_fwd_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_add_row_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_add_col_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_add_scores_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32]),
    "hnh_attn_add_pack_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32]),
    "hnh_attn_add_update_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32]),
}
ATTN_ADD_MAX_F = 256  # HNH_ATTN_ADD_MAX_F


def attn_add_scored_width(f: int) -> int:
    """HNH_ATTN_ADD_SCORED_WIDTH: [A (0) | s t]"""
    return f + (f & 1) + 2


def attn_add_packed_width(f: int) -> int:
    """HNH_ATTN_ADD_PACKED_WIDTH: [dZ (0) | s lse delta 0]"""
    return f + (f & 1) + 4


class AttnAdd(C.Structure):
    """struct hnh_attn_add"""
    _fields_ = [("M", _vp), ("ld_m", _i64), ("dZ", _vp), ("ld_dz", _i64), ("lse", _vp), ("delta", _vp), ("Y", _vp), ("ld_y", _i64),
                ("Out", _vp), ("ld_out", _i64), ("vec", _vp), ("ld_vec", _i64), ("row_max", _vp), ("row_sum", _vp), ("relu_dst", _vp),
                ("relu_ld", _i64), ("f", _i32), ("leaky_alpha", _dbl)]


# include/hnh_attn_dropout.h: attention and feature dropout of the GAT with masks from a keyed counter-based generator; a fifth OPTIONAL
# group bound only for the product library
ATTN_DROP_SIGNATURES = {
    "hnh_attn_drop_fwd_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_drop_row_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_drop_col_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_drop_scores_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i64, _i32]),
    "hnh_attn_drop_pack_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i64, _i32]),
    "hnh_feat_drop_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, C.c_uint64, C.c_uint32, C.c_uint32, _dbl, _i32]),
    "hnh_dropout_words_u32": (_i32, [_vp, _vp, _vp, _vp, _i64, C.c_uint64, C.c_uint32, C.c_uint32, _i32]),
}
DROPOUT_STREAM_ATTENTION, DROPOUT_STREAM_FEATURE = 0, 1  # HNH_DROPOUT_STREAM_*


def attn_drop_scored_width(f: int) -> int:
    """HNH_ATTN_DROP_SCORED_WIDTH: [A (0) | s t | id 0]"""
    return f + (f & 1) + 4


def dropout_threshold(p: float) -> int:
    """floor(p * 2^32): an entry is kept iff its word is >= this"""
    return int(np.floor(p * 4294967296.0))


class AttnDrop(C.Structure):
    """struct hnh_attn_drop"""
    _fields_ = [("seed", C.c_uint64), ("w2", C.c_uint32), ("threshold", C.c_uint32), ("scale", _dbl), ("row_id0", _i64)]


# include/hnh_train.h: the training step's cross-entropy head and table-driven optimizer; a sixth OPTIONAL group bound only for the
# product library
TRAIN_SIGNATURES = {
    "hnh_xent_rows_f64_workspace": (_i64, [_i64]),
    "hnh_xent_rows_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _dbl, _vp, _i64, _vp, _vp, _i64, _i32]),
    "hnh_optim_step_f64": (_i32, [_vp, _vp, _i32, _vp, _i32]),
}
XENT_MAX_WIDTH = 4096  # HNH_XENT_MAX_WIDTH
OPTIM_ADAM, OPTIM_SGD, OPTIM_MAX_TENSORS = 0, 1, 32  # HNH_OPTIM_*


# include/hnh_train_multilabel.h: the multi-label (sigmoid) head of the training step; a further OPTIONAL group bound only for the product
# library
MULTILABEL_SIGNATURES = {
    "hnh_bce_rows_f64_workspace": (_i64, [_i64]),
    "hnh_bce_rows_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _dbl, _vp, _i64, _vp, _vp, _i64, _i32]),
}


# include/hnh_train_clip.h: gradient clipping by global norm and AdamW (the sum of squares of a table of gradients, and the optimizer step
# with a clip coefficient from device memory); a further OPTIONAL group bound only for the product library
TRAIN_CLIP_SIGNATURES = {
    "hnh_grad_sumsq_f64_workspace": (_i64, [_vp, _i32]),
    "hnh_grad_sumsq_f64": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32]),
    "hnh_optim_step_clip_f64": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _dbl, _i32]),
}
OPTIM_ADAMW, CLIP_MAX_SUMS = 2, 8  # HNH_OPTIM_ADAMW, HNH_CLIP_MAX_SUMS


# include/hnh_als_implicit.h: the Gram term and the guarded CG update of implicit-feedback ALS (api.ImplicitALS); a further OPTIONAL group
# bound only for the product library
ALS_IMPLICIT_SIGNATURES = {
    "hnh_gram_rows_f64": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32]),
}
GRAM_MAX_R = 256  # HNH_GRAM_MAX_R


# include/hnh_topk.h: top-k recommendation for implicit-feedback ALS (api.ImplicitALS.recommend): scores and selection in one kernel, the
# merge of lists and a row gather; a further OPTIONAL group bound only for the product library
TOPK_SIGNATURES = {
    "hnh_topk_rows_f64_workspace": (_i64, [_i64, _i64, _i32, _i32]),
    "hnh_topk_rows_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _i32]),
    "hnh_topk_merge_f64": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _i32]),
    "hnh_take_rows_f64": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i32]),
}
TOPK_MAX_K, TOPK_MAX_R, TOPK_MAX_SPLITS = 128, 512, 1024  # HNH_TOPK_MAX_*


# include/hnh_rank.h: exact item ranks for implicit-feedback ALS (api.ImplicitALS.rank_of): counting on the score tile, the scores of single
# pairs and the subtraction of excluded entries; a further OPTIONAL group bound only for the product library.  tgt_ptr of hnh_rank_rows_f64
# is a HOST array.
RANK_SIGNATURES = {
    "hnh_pair_scores_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i32]),
    "hnh_rank_rows_f64_workspace": (_i64, [_i64, _i64, _i64, _i32]),
    "hnh_rank_rows_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i32]),
    "hnh_rank_exclude_f64": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
}
RANK_MAX_R, RANK_MAX_TARGETS, RANK_MAX_SPLITS = 512, 16, 1024  # HNH_RANK_MAX_*


class GramCg(C.Structure):
    """struct hnh_gram_cg"""
    _fields_ = [("x", _vp), ("r", _vp), ("p", _vp), ("rs", _vp)]


class OptimTensor(C.Structure):
    """struct hnh_optim_tensor"""
    _fields_ = [("p", _vp), ("ld_p", _i64), ("g", _vp), ("ld_g", _i64), ("m", _vp), ("v", _vp), ("rows", _i64), ("cols", _i64)]


class Optim(C.Structure):
    """struct hnh_optim"""
    _fields_ = [("kind", _i32), ("reserved", _i32), ("lr", _dbl), ("beta1", _dbl), ("beta2", _dbl), ("eps", _dbl), ("momentum", _dbl),
                ("weight_decay", _dbl), ("bias1", _dbl), ("bias2", _dbl)]


# include/hnh_attn_v2.h: GATv2 dynamic attention scores of the GAT, forward and backward; a seventh OPTIONAL group bound only for the
# product library.  The column pass gathers the packed operand of include/hnh_attn_grad.h (attn_grad_packed_width(f, True)).
V2_SIGNATURES = {
    "hnh_attn_v2_fwd_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_v2_row_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_v2_col_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_v2_finish_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i32]),
}
ATTN_V2_MAX_F = 256  # HNH_ATTN_V2_MAX_F


def attn_v2_finish_work(f: int) -> int:
    """HNH_ATTN_V2_FINISH_WORK: doubles of workspace of hnh_attn_v2_finish_f64"""
    return 1024 * f


class AttnV2(C.Structure):
    """struct hnh_attn_v2"""
    _fields_ = [("X", _vp), ("ld_x", _i64), ("a", _vp), ("dZ", _vp), ("ld_dz", _i64), ("lse", _vp), ("delta", _vp), ("Y", _vp), ("ld_y", _i64),
                ("Out", _vp), ("ld_out", _i64), ("Out2", _vp), ("ld_out2", _i64), ("row_max", _vp), ("row_sum", _vp), ("relu_dst", _vp),
                ("relu_ld", _i64), ("f", _i32), ("leaky_alpha", _dbl)]


# include/hnh_attn_qkv.h: query/key/value attention scores of the GAT (score "transformer"), forward and backward; a tenth OPTIONAL group
# bound only for the product library.  Every pass gathers a packed operand of include/hnh_attn_grad.h: attn_grad_packed_width(f, False) for
# the forward and the row pass ([K | V]), attn_grad_packed_width(f, True) for the column pass ([Q | dZ | lse delta]).
QKV_SIGNATURES = {
    "hnh_attn_qkv_fwd_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_qkv_row_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_qkv_col_csr_p": (_i32, [_vp, _vp, _vp, C.c_uint, _vp, _i32]),
}
ATTN_QKV_MAX_F = 256  # HNH_ATTN_QKV_MAX_F


class AttnQKV(C.Structure):
    """struct hnh_attn_qkv"""
    _fields_ = [("X", _vp), ("ld_x", _i64), ("X2", _vp), ("ld_x2", _i64), ("dZ", _vp), ("ld_dz", _i64), ("lse", _vp), ("delta", _vp), ("Y", _vp),
                ("ld_y", _i64), ("Out", _vp), ("ld_out", _i64), ("Out2", _vp), ("ld_out2", _i64), ("row_max", _vp), ("row_sum", _vp),
                ("relu_dst", _vp), ("relu_ld", _i64), ("values", _vp), ("f", _i32), ("scale", _dbl)]


# include/hnh_attn_edge.h: a per-edge bias on the logits of the query/key/value attention (GAT.set_edge_bias); an eleventh OPTIONAL group bound
# only for the product library.  The three passes of QKV_SIGNATURES with `const double* bias` behind the arguments: bias[e] belongs to entry e
# of the block's CSR order.
EDGE_SIGNATURES = {
    "hnh_attn_qkv_bias_fwd_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_qkv_bias_row_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_qkv_bias_col_csr_p": (_i32, [_vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
}


# include/hnh_attn_edge_grad.h: the gradient of that bias (GAT.set_edge_bias_learned); a twelfth OPTIONAL group bound only for the product
# library.  The two backward passes of EDGE_SIGNATURES with `double* dbias, int accumulate` behind the bias: dbias[e] is addressed like bias[e].
EDGE_GRAD_SIGNATURES = {
    "hnh_attn_qkv_bias_grad_row_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _i32]),
    "hnh_attn_qkv_bias_grad_col_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _vp, _i32]),
}


# include/hnh_attn_coef.h: export of the GAT's per-edge attention coefficients in every score mode; an eighth OPTIONAL group bound only for the
# product library
ATTN_COEF_SIGNATURES = {
    "hnh_attn_coef_csr_p": (_i32, [_vp, _vp, _vp, _vp, _vp, C.c_uint, _vp, _i32]),
    "hnh_attn_coef_scores_f64": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i64, _i32]),
}
ATTN_COEF_MAX_F = 256  # HNH_ATTN_COEF_MAX_F
ATTN_COEF_PAIR_WIDTH = 2  # HNH_ATTN_COEF_PAIR_WIDTH: [t | id]
ATTN_COEF_DOT, ATTN_COEF_ADDITIVE, ATTN_COEF_GATV2 = 0, 1, 2  # HNH_ATTN_COEF_*


# include/hnh_gat_skip.h: bias and skip connections of the GAT layers (the addend flag of the finishing calls and three dense kernels); a
# ninth OPTIONAL group bound only for the product library
SKIP_SIGNATURES = {
    "hnh_skip_addend_cols_f64": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32]),
    "hnh_skip_grad_cols_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32]),
    "hnh_colsum_f64_workspace": (_i64, [_i64, _i64]),
    "hnh_colsum_f64": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i32]),
}
ATTN_ADDEND = 0x40  # HNH_ATTN_ADDEND: the finishing call adds what waits in relu_dst before the activation


# include/hnh_gat_norm.h: layer normalisation of the GAT layers (two dense row passes and the backward pass's workspace size); a further
# OPTIONAL group bound only for the product library
NORM_SIGNATURES = {
    "hnh_layernorm_fwd_f64": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _dbl, _i32, _i32]),
    "hnh_layernorm_bwd_workspace": (_i64, [_i64, _i64]),
    "hnh_layernorm_bwd_f64": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i32]),
}
NORM_MAX_COLS = 4096  # HNH_NORM_MAX_COLS


class AttnCoef(C.Structure):
    """struct hnh_attn_coef"""
    _fields_ = [("X", _vp), ("ld_x", _i64), ("a", _vp), ("s", _vp), ("lse", _vp), ("Y", _vp), ("ld_y", _i64), ("f", _i32), ("score", _i32),
                ("leaky_alpha", _dbl)]


class AttnState(C.Structure):
    """struct hnh_attn_state"""
    _fields_ = [("row_max", _vp), ("row_sum", _vp), ("lse", _vp), ("leaky_alpha", _dbl), ("relu_dst", _vp), ("relu_ld", _i64)]


class CsrBlock(C.Structure):
    """struct hnh_csr_block"""
    _fields_ = [("rows", C.c_int64), ("nnz", C.c_int64), ("cols", C.c_int64), ("max_row_nnz", C.c_int32), ("reserved", C.c_int32),
                ("rowptr", C.c_void_p), ("col_idx", C.c_void_p), ("plan", C.c_void_p)]

class CgUpdate(C.Structure):
    """struct hnh_cg_update"""
    _fields_ = [("x", C.c_void_p), ("r", C.c_void_p), ("p", C.c_void_p), ("rsold", C.c_void_p), ("eps", C.c_double)]


class FusedExtras(C.Structure):
    """struct hnh_fused_extras"""
    _fields_ = [("leaky_alpha", C.c_double), ("x_scale", C.c_double), ("rowdot", C.c_void_p), ("cg", C.POINTER(CgUpdate)),
                ("relu_dst", C.c_void_p), ("relu_ld", C.c_int64)]


class TupleKey(C.Structure):
    """struct hnh_tuple_key"""
    _fields_ = [("kind", C.c_int), ("transpose", C.c_int), ("rows_in_block", C.c_int64), ("cols_in_block", C.c_int64),
                ("n_col_blocks", C.c_int64), ("owner_table", C.c_void_p), ("div", C.c_int64)]


KEY_ROW_COL, KEY_COL_ROW, KEY_OWNER, KEY_COL_DIV = 0, 1, 2, 3
TUPLE_DTYPE = [("r", "<u8"), ("c", "<u8"), ("value", "<f8")]  # struct hnh_tuple


class CsrWindow(C.Structure):
    """struct hnh_csr_window"""
    _fields_ = [("beg", _vp), ("end", _vp), ("last", _i32)]


_lib = None


def load(path: str | None = None) -> C.CDLL:
    """dlopen the HIP kernel library and bind every declared symbol (raises if any is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError("HIP kernel library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
    # One HIP runtime per process: PyTorch bundles its own libamdhip64/librccl (same SONAMEs as
    # /opt/rocm's).  If torch is going to be used (bench.py, torch.distributed bootstrap) it must be
    # imported BEFORE this library so that both bind to the same runtime; loading in the other order
    # leaves two allocators fighting at process exit.
    if os.environ.get("HNH_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(p)  # RTLD_LOCAL: the oracle test double exports the same symbol names
    for name, (res, args) in list(SIGNATURES.items()) + list(AIDS_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if path is None or os.path.abspath(p) == os.path.abspath(LIB_PATH):
        for name, (res, args) in list(GRAD_SIGNATURES.items()) + list(ATTN_SIGNATURES.items()) + list(ATTN_GRAD_SIGNATURES.items()) + \
                list(ATTN_ADD_SIGNATURES.items()) + list(ATTN_DROP_SIGNATURES.items()) + list(TRAIN_SIGNATURES.items()) + \
                list(V2_SIGNATURES.items()) + list(ATTN_COEF_SIGNATURES.items()) + list(SKIP_SIGNATURES.items()) + \
                list(QKV_SIGNATURES.items()) + list(EDGE_SIGNATURES.items()) + list(EDGE_GRAD_SIGNATURES.items()) + \
                list(NORM_SIGNATURES.items()) + list(MULTILABEL_SIGNATURES.items()) + list(TRAIN_CLIP_SIGNATURES.items()) + \
                list(ALS_IMPLICIT_SIGNATURES.items()) + list(TOPK_SIGNATURES.items()) + list(RANK_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = lib
    return lib


class HnhError(RuntimeError):
    pass


class Ctx:
    """One hnh_ctx (device + compute/comm streams).  Raises if there is no GPU."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _vp()
        rc = self.lib.hnh_ctx_create(device, C.byref(h))
        if rc != OK:
            raise HnhError("hnh_ctx_create(device=%d) failed with status %d: no usable MI355X (HIP) device" % (device, rc))
        self.h = h

    def check(self, rc: int, what: str = ""):
        if rc != OK:
            raise HnhError("%s failed (%d): %s" % (what, rc, self.lib.hnh_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.hnh_ctx_destroy(self.h)
            self.h = None

    # ---- memory helpers
    def alloc(self, nbytes: int) -> int:
        p = _vp()
        self.check(self.lib.hnh_malloc(self.h, nbytes, C.byref(p)), "hnh_malloc")
        return p.value

    def free(self, ptr: int):
        self.check(self.lib.hnh_free(self.h, ptr), "hnh_free")

    def upload(self, arr: np.ndarray) -> "DevArray":
        return DevArray.from_host(self, arr)

    def sync(self, stream: int = STREAM_COMPUTE):
        self.check(self.lib.hnh_stream_sync(self.h, stream), "hnh_stream_sync")


class DevArray:
    """A typed device allocation owned by Python (test / bench plumbing only)."""

    def __init__(self, ctx: Ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = ctx.alloc(self.nbytes)

    @classmethod
    def from_host(cls, ctx: Ctx, arr: np.ndarray) -> "DevArray":
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.shape, arr.dtype)
        d.set(arr)
        return d

    def set(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes
        self.ctx.check(self.ctx.lib.hnh_memcpy(self.ctx.h, self.ptr, arr.ctypes.data, self.nbytes, H2D, STREAM_COMPUTE), "h2d")
        self.ctx.sync()

    def get(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        self.ctx.sync()
        self.ctx.check(self.ctx.lib.hnh_memcpy(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes, D2H, STREAM_COMPUTE), "d2h")
        self.ctx.sync()
        return out

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = None
