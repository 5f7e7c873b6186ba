"""ctypes binding of include/hnh_dist.h (lib/libhnh_host.so): the HnH operator surface for Python callers.

Pure plumbing for tests/ and bench.py — the schedules, sparse storage and transports are C++
(csrc/host), the kernels are HIP (csrc/hip).  Method names follow the reference's classes
(Distributed_Sparse::sddmmA / spmmA / fusedSpMM / like_A_matrix ..., distributed_sparse.h:32-388).
There is no compute path in Python and no CPU fallback: with the default backend every constructor
below raises unless the HIP library loads and a GPU is present.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import threading

import numpy as np

from . import _kernels

HERE = os.path.dirname(os.path.abspath(__file__))
# HNH_HOST_LIB_DEV: the measurement tools load libhnh_host_aids.so (the same library + the paced stand-ins, see
# include/hnh_measurement_aids.h); nothing else sets it
HOST_LIB = os.environ.get("HNH_HOST_LIB_DEV") or os.path.join(HERE, "lib", "libhnh_host.so")

K_SDDMM_A, K_SPMM_A, K_SPMM_B, K_SDDMM_B = 0, 1, 2, 3
AMAT, BMAT = 0, 1
ALGORITHMS = ("15d_fusion1", "15d_fusion2", "15d_sparse", "25d_dense_replicate", "25d_sparse_replicate")

_vp, _i32, _i64, _dbl, _sz, _u64 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t, C.c_uint64
_pi64, _pdbl, _pvp, _pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_int)

SENDRECV_CB = C.CFUNCTYPE(_i32, _vp, _vp, _sz, _i32, _vp, _sz, _i32)
BARRIER_CB = C.CFUNCTYPE(_i32, _vp)
ALLGATHER_CB = C.CFUNCTYPE(_i32, _vp, _vp, _vp, _sz)


class CommCallbacks(C.Structure):
    _fields_ = [("user", _vp), ("sendrecv", SENDRECV_CB), ("barrier", BARRIER_CB), ("allgather", ALLGATHER_CB)]


SIGNATURES = {
    "hnh_host_last_error": (C.c_char_p, []),
    "hnh_backend_load": (_i32, [C.c_char_p]),
    "hnh_host_backend_name": (C.c_char_p, []),
    "hnh_world_create_single": (_i32, [_i32, _pvp]),
    "hnh_thread_group_create": (_i32, [_i32, _pvp]),
    "hnh_thread_group_destroy": (_i32, [_vp]),
    "hnh_world_create_thread": (_i32, [_vp, _i32, _i32, _pvp]),
    "hnh_rccl_unique_id": (_i32, [_vp]),
    "hnh_world_create_rccl": (_i32, [_i32, _i32, _i32, _vp, _pvp]),
    "hnh_world_create_ipc": (_i32, [_i32, _i32, _i32, C.c_char_p, _pvp]),
    "hnh_world_create_callback": (_i32, [_i32, _i32, _i32, C.POINTER(CommCallbacks), _pvp]),
    "hnh_world_destroy": (_i32, [_vp]),
    "hnh_world_rank": (_i32, [_vp]),
    "hnh_world_size": (_i32, [_vp]),
    "hnh_world_barrier": (_i32, [_vp]),
    "hnh_world_sync": (_i32, [_vp]),
    "hnh_world_set_timing_sync": (_i32, [_vp, _i32]),
    "hnh_world_set_solo": (_i32, [_vp, _i32]),
    "hnh_world_stream": (_vp, [_vp, _i32]),
    "hnh_world_ctx": (_vp, [_vp]),
    "hnh_world_grid_probe": (_i32, [_vp, _i32, _i32, _i32, _i32, _pi32, _pi32]),
    "hnh_world_preflight": (_i32, [_vp, _i32, _i64, C.POINTER(_dbl)]),
    "hnh_world_split_signature": (_i32, [_vp, C.POINTER(_u64), _pi32]),
    "hnh_world_identities": (_i32, [_vp, _vp]),
    "hnh_spmat_create": (_i32, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _pvp]),
    "hnh_spmat_load_tuples": (_i32, [_vp, _i32, _i32, _i32, C.c_char_p, _pvp]),
    "hnh_spmat_info": (_i32, [_vp, _pi64]),
    "hnh_spmat_permute": (_i32, [_vp, _u64]),
    "hnh_spmat_destroy": (_i32, [_vp]),
    "hnh_er_generate": (_i32, [_u64, _u64, _u64, _u64, _pvp, _pi64]),
    "hnh_rmat_generate": (_i32, [_i32, _u64, _dbl, _dbl, _dbl, _u64, _i32, _pvp, _pi64]),
    "hnh_er_fetch": (_i32, [_vp, _vp, _vp]),
    "hnh_write_matrix_market": (_i32, [C.c_char_p, _i64, _i64, _i64, _vp, _vp, _vp, _i32]),
    "hnh_dist_create": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _pvp]),
    "hnh_dist_destroy": (_i32, [_vp]),
    "hnh_dist_info": (_i32, [_vp, _pi64]),
    "hnh_dist_submatrices": (_i32, [_vp, _i32, _vp, _i32]),
    "hnh_dist_set_r": (_i32, [_vp, _i32]),
    "hnh_dist_json": (_i32, [_vp, _i32, C.c_char_p, _sz]),
    "hnh_dist_reset_timers": (_i32, [_vp]),
    "hnh_dist_kernel_profile": (_i32, [_vp, _i32, _pdbl, _pi64]),
    "hnh_dist_borrow_stats": (_i32, [_vp, _pi64]),
    "hnh_dense_create": (_i32, [_vp, _i64, _i64, _dbl, _pvp]),
    "hnh_dense_wrap": (_i32, [_vp, _vp, _i64, _i64, _pvp]),
    "hnh_dense_like": (_i32, [_vp, _i32, _dbl, _pvp]),
    "hnh_dense_shape": (_i32, [_vp, _pi64]),
    "hnh_dense_data": (_vp, [_vp]),
    "hnh_dense_upload": (_i32, [_vp, _vp]),
    "hnh_dense_download": (_i32, [_vp, _vp]),
    "hnh_dense_fill": (_i32, [_vp, _dbl]),
    "hnh_dense_copy": (_i32, [_vp, _vp]),
    "hnh_dense_destroy": (_i32, [_vp]),
    "hnh_dense_dummy_initialize": (_i32, [_vp, _vp, _i32]),
    "hnh_vec_create": (_i32, [_vp, _i64, _dbl, _pvp]),
    "hnh_vec_like": (_i32, [_vp, _i32, _dbl, _pvp]),
    "hnh_vec_size": (_i64, [_vp]),
    "hnh_vec_data": (_vp, [_vp]),
    "hnh_vec_upload": (_i32, [_vp, _vp]),
    "hnh_vec_download": (_i32, [_vp, _vp]),
    "hnh_vec_fill": (_i32, [_vp, _dbl]),
    "hnh_vec_destroy": (_i32, [_vp]),
    "hnh_dist_initial_shift": (_i32, [_vp, _vp, _vp, _i32]),
    "hnh_dist_de_shift": (_i32, [_vp, _vp, _vp, _i32]),
    "hnh_dist_sddmmA": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "hnh_dist_sddmmB": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "hnh_dist_spmmA": (_i32, [_vp, _vp, _vp, _vp]),
    "hnh_dist_spmmB": (_i32, [_vp, _vp, _vp, _vp]),
    "hnh_dist_fusedSpMM": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "hnh_dist_algorithm": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "hnh_dist_hold_moving_operand": (_i32, [_vp, _vp]),
    "hnh_dist_walk_windows_when_held": (_i32, [_vp, _i32]),
    "hnh_dist_fusedSpMM_out": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, C.c_double, C.c_double, _vp, C.POINTER(C.c_int)]),
    "hnh_als_create": (_i32, [_vp, _i32, _u64, _pvp]),
    "hnh_als_destroy": (_i32, [_vp]),
    "hnh_als_set_ground_truth": (_i32, [_vp, _vp, _vp]),
    "hnh_als_initialize_embeddings": (_i32, [_vp]),
    "hnh_als_set_embeddings": (_i32, [_vp, _vp, _vp]),
    "hnh_als_get_embeddings": (_i32, [_vp, _vp, _vp]),
    "hnh_als_cg_optimizer": (_i32, [_vp, _i32, _i32]),
    "hnh_als_run_cg": (_i32, [_vp, _i32]),
    "hnh_als_compute_residual": (_i32, [_vp, _pdbl]),
    "hnh_ials_create": (_i32, [_vp, C.c_double, _u64, _pvp]),
    "hnh_ials_destroy": (_i32, [_vp]),
    "hnh_ials_set_confidence": (_i32, [_vp, _vp, _vp]),
    "hnh_ials_initialize_embeddings": (_i32, [_vp]),
    "hnh_ials_set_embeddings": (_i32, [_vp, _vp, _vp]),
    "hnh_ials_get_embeddings": (_i32, [_vp, _vp, _vp]),
    "hnh_ials_half_step": (_i32, [_vp, _i32, _i32]),
    "hnh_ials_run": (_i32, [_vp, _i32, _i32]),
    "hnh_ials_loss": (_i32, [_vp, _pdbl]),
    "hnh_ials_gram": (_i32, [_vp, _i32, _vp]),
    "hnh_ials_set_folded": (_i32, [_vp, _i32]),
    "hnh_ials_recommend": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "hnh_ials_rank_of": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "hnh_gat_create": (_i32, [_vp, _i32, _pi32, _dbl, _pvp]),
    "hnh_gat_destroy": (_i32, [_vp]),
    "hnh_gat_weight_shape": (_i32, [_vp, _i32, _i32, _pi64]),
    "hnh_gat_set_weight": (_i32, [_vp, _i32, _i32, _vp]),
    "hnh_gat_set_input": (_i32, [_vp, _vp]),
    "hnh_gat_get_output": (_i32, [_vp, _vp]),
    "hnh_gat_buffer_shape": (_i32, [_vp, _i32, _pi64]),
    "hnh_gat_forward": (_i32, [_vp]),
    "hnh_gat_backward": (_i32, [_vp, _vp]),
    "hnh_gat_attention_coefficients": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "hnh_gat_get_weight_grad": (_i32, [_vp, _i32, _i32, _vp]),
    "hnh_gat_get_input_grad": (_i32, [_vp, _vp]),
    "hnh_gat_set_attention": (_i32, [_vp, _i32]),
    "hnh_gat_set_backward": (_i32, [_vp, _i32]),
    "hnh_gat_set_score": (_i32, [_vp, _i32]),
    "hnh_gat_set_qk_weight": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "hnh_gat_get_qk_weight": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "hnh_gat_get_qk_weight_grad": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "hnh_gat_set_edge_bias": (_i32, [_vp, _i32, _vp, _vp]),
    "hnh_gat_set_edge_bias_learned": (_i32, [_vp, _i32, _i32]),
    "hnh_gat_get_edge_bias": (_i32, [_vp, _i32, _i32, _vp]),
    "hnh_gat_get_edge_bias_grad": (_i32, [_vp, _i32, _i32, _vp]),
    "hnh_gat_set_activation": (_i32, [_vp, _i32, _i32]),
    "hnh_gat_set_attn_vectors": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "hnh_gat_set_residual": (_i32, [_vp, _i32, _i32]),
    "hnh_gat_set_residual_weight": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_get_residual_weight": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_get_residual_weight_grad": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_set_bias": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_get_bias": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_get_bias_grad": (_i32, [_vp, _i32, _vp]),
    "hnh_gat_set_norm": (_i32, [_vp, _i32, _i32, C.c_double]),
    "hnh_gat_set_norm_weights": (_i32, [_vp, _i32, _vp, _vp, C.c_int64]),
    "hnh_gat_get_norm_weights": (_i32, [_vp, _i32, _vp, _vp, C.c_int64]),
    "hnh_gat_get_norm_grad": (_i32, [_vp, _i32, _vp, _vp, C.c_int64]),
    "hnh_gat_get_attn_grads": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "hnh_gat_set_dropout": (_i32, [_vp, _dbl, _dbl, C.c_uint64]),
    "hnh_gat_set_dropout_seed": (_i32, [_vp, C.c_uint64]),
    "hnh_gat_get_weight": (_i32, [_vp, _i32, _i32, _vp]),
    "hnh_gat_get_attn_vectors": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "hnh_gat_set_labels": (_i32, [_vp, _vp, _vp, _i64, _i32]),
    "hnh_gat_set_multilabel_targets": (_i32, [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    "hnh_gat_multilabel_counts": (_i32, [_vp, _pdbl, _pdbl, _pdbl]),
    "hnh_gat_loss": (_i32, [_vp, _vp, _i64, _vp, _pdbl, _pdbl]),
    "hnh_gat_set_optimizer": (_i32, [_vp, _i32, _dbl, _dbl, _dbl, _dbl, _dbl, _dbl]),
    "hnh_gat_optimizer_step": (_i32, [_vp]),
    "hnh_gat_set_grad_clip": (_i32, [_vp, _dbl]),
    "hnh_gat_grad_norm": (_i32, [_vp, _pdbl]),
    "hnh_gat_set_learning_rate": (_i32, [_vp, _dbl]),
    "hnh_gat_learning_rate": (_i32, [_vp, _pdbl]),
    "hnh_gat_set_lr_schedule": (_i32, [_vp, _i32, _i64, _i64, _dbl]),
    "hnh_gat_train_step": (_i32, [_vp, _pdbl, _pdbl]),
    "hnh_gat_evaluate": (_i32, [_vp, _vp, _i64, _pdbl, _pdbl]),
    "hnh_dropout_word": (C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
}

_lib = None
_lock = threading.Lock()


class HnhError(RuntimeError):
    pass


def lib() -> C.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(HOST_LIB):
                raise HnhError("host library %s is missing: run __graft_entry__.build()" % HOST_LIB)
            if os.environ.get("HNH_NO_TORCH") != "1":
                try:  # one HIP runtime per process: torch's bundled one must be loaded first if torch is used at all
                    import torch  # noqa: F401
                except ImportError:
                    pass
            l = C.CDLL(HOST_LIB)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(l, name)
                fn.restype, fn.argtypes = res, args
            _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        raise HnhError("%s failed (%d): %s" % (what, rc, lib().hnh_host_last_error().decode(errors="replace")))


def load_backend(path: str | None = None) -> str:
    """Select the implementation of the kernel ABI.  None = the product HIP library (the default).
    Tests pass oracle/liboracle_backend.so explicitly to exercise host logic without a GPU."""
    _check(lib().hnh_backend_load(path.encode() if path else None), "hnh_backend_load")
    return backend_name()


def backend_name() -> str:
    return lib().hnh_host_backend_name().decode()


def generate_er(m: int, n: int, draws: int, seed: int = 12345):
    """The shared synthetic generator (native, OpenMP); bit-identical to oracle.erdos_renyi_mn."""
    h, cnt = _vp(), _i64()
    _check(lib().hnh_er_generate(m, n, draws, seed, C.byref(h), C.byref(cnt)), "hnh_er_generate")
    rows, cols = np.empty(cnt.value, np.int64), np.empty(cnt.value, np.int64)
    _check(lib().hnh_er_fetch(h, rows.ctypes.data, cols.ctypes.data), "hnh_er_fetch")
    return rows, cols


def generate_rmat(logm: int, edges: int, a: float = 0.57, b: float = 0.19, c: float = 0.19, seed: int = 12345, scramble: bool = True):
    """Graph500-style R-MAT (skewed degrees), de-duplicated and sorted row-major; twin of oracle.rmat."""
    h, cnt = _vp(), _i64()
    _check(lib().hnh_rmat_generate(logm, edges, a, b, c, seed, int(scramble), C.byref(h), C.byref(cnt)), "hnh_rmat_generate")
    rows, cols = np.empty(cnt.value, np.int64), np.empty(cnt.value, np.int64)
    _check(lib().hnh_er_fetch(h, rows.ctypes.data, cols.ctypes.data), "hnh_er_fetch")
    return rows, cols


def write_matrix_market(path: str, m: int, n: int, rows, cols, values=None, symmetric: bool = False):
    """hnh_write_matrix_market: the entries as a MatrixMarket coordinate file, formatted by all host cores."""
    rows, cols = np.ascontiguousarray(rows, np.int64), np.ascontiguousarray(cols, np.int64)
    vals = None if values is None else np.ascontiguousarray(values, np.float64)
    _check(lib().hnh_write_matrix_market(path.encode(), m, n, len(rows), rows.ctypes.data, cols.ctypes.data,
                                         None if vals is None else vals.ctypes.data, int(symmetric)), "hnh_write_matrix_market")


# --------------------------------------------------------------------------------------------- worlds
class World:
    def __init__(self, handle, keepalive=None):
        self.h = handle
        self._keep = keepalive
        self.rank = lib().hnh_world_rank(handle)
        self.size = lib().hnh_world_size(handle)

    @classmethod
    def single(cls, device: int = 0) -> "World":
        h = _vp()
        _check(lib().hnh_world_create_single(device, C.byref(h)), "hnh_world_create_single")
        return cls(h)

    @classmethod
    def thread(cls, group: "ThreadGroup", rank: int, device: int = 0) -> "World":
        h = _vp()
        _check(lib().hnh_world_create_thread(group.h, rank, device, C.byref(h)), "hnh_world_create_thread")
        return cls(h, group)

    @classmethod
    def rccl(cls, rank: int, nranks: int, device: int, unique_id: bytes) -> "World":
        h = _vp()
        buf = C.create_string_buffer(unique_id, _kernels.UNIQUE_ID_BYTES)
        _check(lib().hnh_world_create_rccl(rank, nranks, device, buf, C.byref(h)), "hnh_world_create_rccl")
        return cls(h)

    @classmethod
    def ipc(cls, rank: int, nranks: int, device: int, session: str) -> "World":
        """One process per GPU of one node, no RCCL: receivers pull out of their peers' mapped buffers.  `session` is the same
        string on every rank (ipc_session_id() on rank 0, handed round by the launcher)."""
        h = _vp()
        _check(lib().hnh_world_create_ipc(rank, nranks, device, session.encode(), C.byref(h)), "hnh_world_create_ipc")
        return cls(h)

    @classmethod
    def callback(cls, rank: int, nranks: int, device: int, callbacks: CommCallbacks) -> "World":
        h = _vp()
        _check(lib().hnh_world_create_callback(rank, nranks, device, C.byref(callbacks), C.byref(h)), "hnh_world_create_callback")
        return cls(h, callbacks)

    def barrier(self):
        _check(lib().hnh_world_barrier(self.h), "barrier")

    def sync(self):
        _check(lib().hnh_world_sync(self.h), "sync")

    def set_solo(self, on: bool):
        """World::set_solo — solo replay (measurement entry point, loopback transport): this rank runs its side of every collective alone."""
        _check(lib().hnh_world_set_solo(self.h, int(on)), "set_solo")

    def set_timing_sync(self, on: bool):
        lib().hnh_world_set_timing_sync(self.h, int(on))

    def grid_probe(self, nr, nc, nh, adjacency):
        out, ok = (C.c_int * 9)(), C.c_int()
        _check(lib().hnh_world_grid_probe(self.h, nr, nc, nh, adjacency, out, C.byref(ok)), "grid_probe")
        return list(out), bool(ok.value)

    PREFLIGHT = ("ring sendrecv", "mesh group (n-1 pairs)", "allgather (layer)", "reduce_scatter (layer)", "allreduce (layer)",
                 "allgatherv + reduce_scatter_v", "device alltoallv", "allgather (world, native)", "reduce_scatter (world, native)")

    def preflight(self, what: int, count: int = 4096) -> float:
        """hnh_world_preflight: one transport primitive on known data; returns the largest deviation (collective)."""
        err = _dbl()
        _check(lib().hnh_world_preflight(self.h, what, count, C.byref(err)), "preflight: " + self.PREFLIGHT[what])
        return err.value

    def identities(self):
        """Collective: where every rank of the world runs — [{"rank", "pid", "device_ordinal", "pci_bus_id", + "comm_count", "comm_rank",
        "comm_device" when the transport has a communicator (RCCL)}], the same list on every rank (hnh_world_identities)."""
        class Rec(C.Structure):
            _fields_ = [("rank", _i32), ("pid", _i32), ("device_ordinal", _i32), ("comm_count", _i32), ("comm_rank", _i32), ("comm_device", _i32),
                        ("pci_bus_id", C.c_char * 40)]
        n = lib().hnh_world_size(self.h)
        buf = (Rec * n)()
        _check(lib().hnh_world_identities(self.h, C.cast(buf, _vp)), "identities")
        out = []
        for r in buf:
            rec = {"rank": r.rank, "pid": r.pid, "device_ordinal": r.device_ordinal, "pci_bus_id": r.pci_bus_id.decode("ascii", "replace")}
            if r.comm_count != -1:  # (-1: the transport has no communicator; -2: RCCL would not say)
                rec.update(comm_count=r.comm_count, comm_rank=r.comm_rank, comm_device=r.comm_device)
            out.append(rec)
        return out

    def split_signature(self):
        sig, n = _u64(), _i32()
        _check(lib().hnh_world_split_signature(self.h, C.byref(sig), C.byref(n)), "split_signature")
        return int(sig.value), int(n.value)

    def close(self):
        if self.h:
            _check(lib().hnh_world_destroy(self.h), "world_destroy")
            self.h = None


def ipc_session_id() -> str:
    """A name no other job on this node uses (made on rank 0, given to every rank)."""
    import os
    import time
    return "%d_%x" % (os.getpid(), time.time_ns())


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(_kernels.UNIQUE_ID_BYTES)
    _check(lib().hnh_rccl_unique_id(buf), "hnh_rccl_unique_id")
    return buf.raw


class ThreadGroup:
    def __init__(self, nranks: int):
        self.h = _vp()
        self.n = nranks
        _check(lib().hnh_thread_group_create(nranks, C.byref(self.h)), "thread_group_create")

    def close(self):
        if self.h:
            lib().hnh_thread_group_destroy(self.h)
            self.h = None


def run_spmd(nranks: int, fn, device: int = 0):
    """Run fn(world) on `nranks` logical ranks = host threads sharing one device (loopback transport).
    Returns the list of results; re-raises the first exception."""
    group = ThreadGroup(nranks)
    results, errors = [None] * nranks, [None] * nranks

    def body(r):
        w = None
        try:
            w = World.thread(group, r, device)
            results[r] = fn(w)
        except BaseException as e:  # noqa: BLE001
            errors[r] = e
        finally:
            if w is not None and errors[r] is None:
                try:
                    w.close()
                except BaseException as e:  # noqa: BLE001
                    errors[r] = e

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    alive = [t for t in threads if t.is_alive()]
    for e in errors:
        if e is not None:
            raise e
    if alive:
        raise HnhError("SPMD ranks hung (a peer probably failed)")
    group.close()
    return results


# --------------------------------------------------------------------------------------------- data
class Dense:
    def __init__(self, world: World, handle):
        self.w, self.h = world, handle

    @classmethod
    def create(cls, world: World, rows: int, cols: int, fill: float = 0.0) -> "Dense":
        h = _vp()
        _check(lib().hnh_dense_create(world.h, rows, cols, fill, C.byref(h)), "dense_create")
        return cls(world, h)

    @classmethod
    def wrap(cls, world: World, device_ptr: int, rows: int, cols: int) -> "Dense":
        h = _vp()
        _check(lib().hnh_dense_wrap(world.h, device_ptr, rows, cols, C.byref(h)), "dense_wrap")
        return cls(world, h)

    @property
    def shape(self):
        o = (C.c_int64 * 2)()
        lib().hnh_dense_shape(self.h, o)
        return int(o[0]), int(o[1])

    @property
    def data_ptr(self) -> int:
        return lib().hnh_dense_data(self.h)

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        assert arr.shape == self.shape, (arr.shape, self.shape)
        _check(lib().hnh_dense_upload(self.h, arr.ctypes.data), "dense_upload")

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        _check(lib().hnh_dense_download(self.h, out.ctypes.data), "dense_download")
        return out

    def fill(self, v: float):
        _check(lib().hnh_dense_fill(self.h, v), "dense_fill")

    def copy_from(self, other: "Dense"):
        _check(lib().hnh_dense_copy(self.h, other.h), "dense_copy")

    def free(self):
        if self.h:
            _check(lib().hnh_dense_destroy(self.h), "dense_destroy")
            self.h = None


class Vec:
    def __init__(self, world: World, handle):
        self.w, self.h = world, handle

    @classmethod
    def create(cls, world: World, n: int, fill: float = 0.0) -> "Vec":
        h = _vp()
        _check(lib().hnh_vec_create(world.h, n, fill, C.byref(h)), "vec_create")
        return cls(world, h)

    def __len__(self):
        return int(lib().hnh_vec_size(self.h))

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        assert arr.size == len(self)
        _check(lib().hnh_vec_upload(self.h, arr.ctypes.data), "vec_upload")

    def download(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.float64)
        _check(lib().hnh_vec_download(self.h, out.ctypes.data), "vec_download")
        return out

    def fill(self, v: float):
        _check(lib().hnh_vec_fill(self.h, v), "vec_fill")

    def free(self):
        if self.h:
            _check(lib().hnh_vec_destroy(self.h), "vec_destroy")
            self.h = None


class SpmatLocal:
    """SpmatLocal (SpmatLocal.hpp:267-606): the tuples this rank holds before redistribution."""

    def __init__(self, world: World, handle):
        self.w, self.h = world, handle

    @classmethod
    def from_tuples(cls, world: World, m: int, n: int, dist_nnz: int, rows, cols, vals=None) -> "SpmatLocal":
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        v = None if vals is None else np.ascontiguousarray(vals, dtype=np.float64)
        h = _vp()
        _check(lib().hnh_spmat_create(world.h, m, n, dist_nnz, len(rows), rows.ctypes.data, cols.ctypes.data,
                                      None if v is None else v.ctypes.data, C.byref(h)), "spmat_create")
        return cls(world, h)

    @classmethod
    def from_global(cls, world: World, m: int, n: int, rows, cols, vals=None) -> "SpmatLocal":
        """Every rank passes the same global tuple list and keeps the strided slice e % p == rank."""
        sl = slice(world.rank, None, world.size)
        return cls.from_tuples(world, m, n, len(rows), rows[sl], cols[sl], None if vals is None else vals[sl])

    @classmethod
    def load_tuples(cls, world: World, read_from_file: bool, log_m: int, nnz_per_row: int, filename: str = "") -> "SpmatLocal":
        h = _vp()
        _check(lib().hnh_spmat_load_tuples(world.h, int(read_from_file), log_m, nnz_per_row, filename.encode(), C.byref(h)),
               "spmat_load_tuples")
        return cls(world, h)

    def permute(self, seed: int):
        """Seeded random relabelling of rows/columns (load balance on real graphs)."""
        _check(lib().hnh_spmat_permute(self.h, seed), "spmat_permute")

    def info(self):
        o = (C.c_int64 * 4)()
        lib().hnh_spmat_info(self.h, o)
        return {"M": int(o[0]), "N": int(o[1]), "dist_nnz": int(o[2]), "local_nnz": int(o[3])}

    def free(self):
        if self.h:
            _check(lib().hnh_spmat_destroy(self.h), "spmat_destroy")
            self.h = None


class DistributedSparse:
    """A Distributed_Sparse subclass chosen by name as in benchmark_dist.cpp:45-82, plus its StandardKernel."""

    def __init__(self, world: World, alg: str, spmat: SpmatLocal, r: int, c: int):
        self.w, self.alg = world, alg
        self.h = _vp()
        _check(lib().hnh_dist_create(world.h, alg.encode(), spmat.h, r, c, C.byref(self.h)), "dist_create(%s)" % alg)

    def info(self) -> dict:
        o = (C.c_int64 * 16)()
        _check(lib().hnh_dist_info(self.h, o), "dist_info")
        names = ["M", "N", "R", "p", "c", "localArows", "localAcols", "localBrows", "localBcols", "nS", "nST", "r_split",
                 "dist_nnz", "proc_rank", "nAsub", "nBsub"]
        return {k: int(v) for k, v in zip(names, o)}

    def submatrices(self, matmode: int) -> np.ndarray:
        n = self.info()["nAsub" if matmode == AMAT else "nBsub"]
        out = np.empty((n, 4), dtype=np.int64)
        _check(lib().hnh_dist_submatrices(self.h, matmode, out.ctypes.data, n), "dist_submatrices")
        return out

    def like_A_matrix(self, v: float = 0.0) -> Dense:
        h = _vp()
        _check(lib().hnh_dense_like(self.h, AMAT, v, C.byref(h)), "like_A_matrix")
        return Dense(self.w, h)

    def like_B_matrix(self, v: float = 0.0) -> Dense:
        h = _vp()
        _check(lib().hnh_dense_like(self.h, BMAT, v, C.byref(h)), "like_B_matrix")
        return Dense(self.w, h)

    def like_S_values(self, v: float = 0.0) -> Vec:
        h = _vp()
        _check(lib().hnh_vec_like(self.h, 0, v, C.byref(h)), "like_S_values")
        return Vec(self.w, h)

    def like_ST_values(self, v: float = 0.0) -> Vec:
        h = _vp()
        _check(lib().hnh_vec_like(self.h, 1, v, C.byref(h)), "like_ST_values")
        return Vec(self.w, h)

    def setRValue(self, r: int):
        _check(lib().hnh_dist_set_r(self.h, r), "setRValue")

    def dummyInitialize(self, m: Dense, matmode: int):
        _check(lib().hnh_dense_dummy_initialize(self.h, m.h, matmode), "dummyInitialize")

    def initial_shift(self, a: Dense | None, b: Dense | None, mode: int):
        _check(lib().hnh_dist_initial_shift(self.h, a.h if a else None, b.h if b else None, mode), "initial_shift")

    def de_shift(self, a: Dense | None, b: Dense | None, mode: int):
        _check(lib().hnh_dist_de_shift(self.h, a.h if a else None, b.h if b else None, mode), "de_shift")

    def sddmmA(self, a, b, s, result):
        _check(lib().hnh_dist_sddmmA(self.h, a.h, b.h, s.h, result.h), "sddmmA")

    def sddmmB(self, a, b, s, result):
        _check(lib().hnh_dist_sddmmB(self.h, a.h, b.h, s.h, result.h), "sddmmB")

    def spmmA(self, a, b, s):
        _check(lib().hnh_dist_spmmA(self.h, a.h, b.h, s.h), "spmmA")

    def spmmB(self, a, b, s):
        _check(lib().hnh_dist_spmmB(self.h, a.h, b.h, s.h), "spmmB")

    def fusedSpMM(self, a, b, s, buf, matmode: int):
        _check(lib().hnh_dist_fusedSpMM(self.h, a.h, b.h, s.h, buf.h, matmode), "fusedSpMM")

    def _coordinates(self, transposed: bool):
        """Two probe SDDMMs at the operator's own R (nothing is changed, nothing is cached): the first with A[i, 0] = i, B[j, 0] = 1 gives every
        value slot its global row of S, the second with A[i, 0] = 1, B[j, 0] = j its column; each value is one integer below max(M, N), exact in
        fp64 for any M, N (no i * N + j product is formed)."""
        def fill(subs, shape, ramp):
            loc = np.zeros(shape)
            flat, off = loc.reshape(-1), 0
            for top, left, rc, cc in subs:
                blk = np.zeros((rc, cc))
                if left <= 0 < left + cc:
                    blk[:, 0 - left] = np.arange(top, top + rc, dtype=np.float64) if ramp else 1.0
                flat[off:off + rc * cc] = blk.reshape(-1)
                off += rc * cc
            return loc

        mode = K_SDDMM_B if transposed else K_SDDMM_A
        like = self.like_ST_values if transposed else self.like_S_values
        a, b, ones = self.like_A_matrix(0.0), self.like_B_matrix(0.0), like(1.0)
        sub_a, sub_b = self.submatrices(AMAT), self.submatrices(BMAT)
        found = []
        try:
            for by_row in (True, False):
                a.upload(fill(sub_a, a.shape, by_row))
                b.upload(fill(sub_b, b.shape, not by_row))
                res = like(0.0)
                try:
                    self.initial_shift(a, b, mode)
                    (self.sddmmB if transposed else self.sddmmA)(a, b, ones, res)
                    self.de_shift(a, b, mode)
                    found.append(np.rint(res.download()).astype(np.int64))
                finally:
                    res.free()
        finally:
            for x in (a, b, ones):
                x.free()
        return found[0], found[1]

    def S_coordinates(self):
        """(rows, cols): int64 arrays with the global coordinates of every entry of a like_S_values vector on this rank, in that vector's
        order, on any schedule (what GAT.attention_coefficients and sddmmA's results are indexed by).  Collective: two SDDMMs at the
        operator's current R, which stays what it was; nothing is cached, so a later setRValue cannot invalidate anything."""
        return self._coordinates(False)

    def ST_coordinates(self):
        """S_coordinates for a like_ST_values vector: (rows, cols) of the entries of S^T, i.e. rows are columns of S and cols rows of S."""
        r, c = self._coordinates(True)
        return c, r

    def hold_moving_operand(self, m=None):
        """Distributed_Sparse::hold_moving_operand(m) / release_moving_operand() (m = None)."""
        _check(lib().hnh_dist_hold_moving_operand(self.h, m.h if m else None), "hold_moving_operand")

    def walk_windows_when_held(self, on=True):
        """Distributed_Sparse::walk_windows_when_held: a held operand's resident blocks are walked by chunk windows, as a fetching call
        does (measurement entry point: one rank's kernel sequence alone on a GPU).  on = 1 / True: adaptive windows (everything has
        landed: one pass); on = 2: one pass per chunk."""
        _check(lib().hnh_dist_walk_windows_when_held(self.h, int(on)), "walk_windows_when_held")

    def fusedSpMM_out(self, a, b, matmode: int, out, leaky_alpha=None, x_scale: float = 0.0, rowdot=None) -> bool:
        """Distributed_Sparse::fusedSpMM_out; False (nothing done) when the schedule has no single fused pass."""
        ok = C.c_int(0)
        _check(lib().hnh_dist_fusedSpMM_out(self.h, a.h, b.h, matmode, out.h, int(leaky_alpha is not None), float(leaky_alpha or 0.0),
                                            float(x_scale), rowdot.h if rowdot else None, C.byref(ok)), "fusedSpMM_out")
        return bool(ok.value)

    def algorithm(self, a, b, s, result, mode: int, initial_replicate: bool):
        _check(lib().hnh_dist_algorithm(self.h, a.h, b.h, s.h, result.h if result else None, mode, int(initial_replicate)), "algorithm")

    def json_algorithm_info(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        _check(lib().hnh_dist_json(self.h, 0, buf, len(buf)), "json_algorithm_info")
        return json.loads(buf.value.decode())

    def json_perf_statistics(self) -> dict:
        buf = C.create_string_buffer(1 << 14)
        _check(lib().hnh_dist_json(self.h, 1, buf, len(buf)), "json_perf_statistics")
        return json.loads(buf.value.decode())

    def reset_performance_timers(self):
        _check(lib().hnh_dist_reset_timers(self.h), "reset_performance_timers")

    def kernel_profile(self, enable: int = -1):
        """enable: 1 start / 0 stop (both reset the counters), -1 just read.  Returns (ms, launches) BEFORE the reset."""
        ms, n = C.c_double(), C.c_int64()
        _check(lib().hnh_dist_kernel_profile(self.h, enable, C.byref(ms), C.byref(n)), "kernel_profile")
        return ms.value, n.value

    def borrow_stats(self):
        """(SpMM arrays lent, SpMM arrays copied, SDDMM results written in place, SDDMM results by a Hadamard pass) — block counts."""
        out = (C.c_int64 * 4)()
        _check(lib().hnh_dist_borrow_stats(self.h, out), "borrow_stats")
        return tuple(out)

    def free(self):
        if self.h:
            _check(lib().hnh_dist_destroy(self.h), "dist_destroy")
            self.h = None


class DistributedALS:
    """Distributed_ALS (als_conjugate_gradients.{h,cpp}): ALS by batched CG around fusedSpMM."""

    def __init__(self, op: DistributedSparse, artificial_groundtruth: bool = False, seed: int = 2022):
        self.op = op
        self.h = _vp()
        _check(lib().hnh_als_create(op.h, int(artificial_groundtruth), seed, C.byref(self.h)), "als_create")

    def set_ground_truth(self, gt_s: Vec, gt_st: Vec):
        _check(lib().hnh_als_set_ground_truth(self.h, gt_s.h, gt_st.h), "als_set_ground_truth")

    def initializeEmbeddings(self):
        _check(lib().hnh_als_initialize_embeddings(self.h), "initializeEmbeddings")

    def set_embeddings(self, a: Dense, b: Dense):
        _check(lib().hnh_als_set_embeddings(self.h, a.h, b.h), "als_set_embeddings")

    def get_embeddings(self, a: Dense, b: Dense):
        _check(lib().hnh_als_get_embeddings(self.h, a.h, b.h), "als_get_embeddings")

    def cg_optimizer(self, matmode: int, cg_max_iter: int):
        _check(lib().hnh_als_cg_optimizer(self.h, matmode, cg_max_iter), "cg_optimizer")

    def run_cg(self, steps: int):
        _check(lib().hnh_als_run_cg(self.h, steps), "run_cg")

    def computeResidual(self) -> float:
        out = C.c_double()
        _check(lib().hnh_als_compute_residual(self.h, C.byref(out)), "computeResidual")
        return out.value

    def free(self):
        if self.h:
            _check(lib().hnh_als_destroy(self.h), "als_destroy")
            self.h = None


class ImplicitALS:
    """Implicit_ALS (csrc/host/als_implicit.hpp): implicit-feedback ALS with confidence weights on a 15d_fusion2 operator.  Preference 1
    with confidence 1 + w on the stored pairs, 0 with confidence 1 everywhere else; every row solved by `iters` guarded CG iterations."""

    def __init__(self, op: DistributedSparse, lam: float, seed: int = 2022):
        self.op = op
        self.h = _vp()
        _check(lib().hnh_ials_create(op.h, float(lam), seed, C.byref(self.h)), "ials_create")

    def set_confidence(self, w_s: Vec, w_st: Vec):
        """w >= 0 per stored pair, in the like_S_values and the like_ST_values layouts"""
        _check(lib().hnh_ials_set_confidence(self.h, w_s.h, w_st.h), "ials_set_confidence")

    def initializeEmbeddings(self):
        _check(lib().hnh_ials_initialize_embeddings(self.h), "ials_initialize_embeddings")

    def set_embeddings(self, a: Dense, b: Dense):
        _check(lib().hnh_ials_set_embeddings(self.h, a.h, b.h), "ials_set_embeddings")

    def get_embeddings(self, a: Dense, b: Dense):
        _check(lib().hnh_ials_get_embeddings(self.h, a.h, b.h), "ials_get_embeddings")

    def half_step(self, matmode: int, iters: int):
        _check(lib().hnh_ials_half_step(self.h, matmode, iters), "ials_half_step")

    def run(self, steps: int, iters: int):
        _check(lib().hnh_ials_run(self.h, steps, iters), "ials_run")

    def loss(self) -> float:
        out = C.c_double()
        _check(lib().hnh_ials_loss(self.h, C.byref(out)), "ials_loss")
        return out.value

    def gram(self, matmode: int) -> np.ndarray:
        """A^T A (AMAT) or B^T B (BMAT), summed over all ranks"""
        r = self.op.info()["R"]
        out = np.empty((r, r), dtype=np.float64)
        _check(lib().hnh_ials_gram(self.h, matmode, out.ctypes.data), "ials_gram")
        return out

    def set_folded(self, folded: bool):
        """True: one hnh_gram_rows_f64 launch adds the Gram term and updates the rows (R <= 256); False: the composed sequence"""
        _check(lib().hnh_ials_set_folded(self.h, int(bool(folded))), "ials_set_folded")

    def recommend(self, users, k: int = 10, filter_seen: bool = True):
        """The first k items of every user (global row numbers, repeats allowed) by <a_u, b_j>, score descending and then item id
        ascending: (ids int64 [nq, k], scores float64 [nq, k]), the tail (-1, -inf) where fewer than k items are left.  filter_seen: the
        items of the user's row of S are never returned.  Collective: every rank passes the same users and gets the same arrays."""
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int64).reshape(-1))
        nq = len(users)
        ids = np.empty((nq, int(k)) if k >= 1 else (nq, 0), dtype=np.int64)
        scores = np.empty(ids.shape, dtype=np.float64)
        _check(lib().hnh_ials_recommend(self.h, users.ctypes.data, nq, int(k), int(bool(filter_seen)), ids.ctypes.data, scores.ctypes.data), "ials_recommend")
        return ids, scores

    def ranking_metrics(self, test_rows, test_cols, k: int = 10, batch: int = 1024) -> dict:
        """precision, map and ndcg at k (the definitions of the `implicit` package's ranking_metrics_at_k) on held-out pairs in global
        coordinates, the same on every rank.  The users are those with a held-out pair; they are recommended in batches with
        filter_seen=True and the sums are kept in numpy on the host.  For a user with held-out set L and list r_1 .. r_k, m = min(k, |L|):
        precision = sum hits / sum m; map = mean of (sum_t [r_t in L] hits_<=t / t) / m; ndcg = mean of sum_t [r_t in L] / log2(t + 1)
        over sum_{t <= m} 1 / log2(t + 1).  Entries with id -1 are misses."""
        test_rows = np.asarray(test_rows, dtype=np.int64).reshape(-1)
        test_cols = np.asarray(test_cols, dtype=np.int64).reshape(-1)
        if len(test_rows) != len(test_cols) or batch < 1:
            raise ValueError("ranking_metrics needs as many rows as columns and batch >= 1")
        order = np.lexsort((test_cols, test_rows))
        rows, cols = test_rows[order], test_cols[order]
        users, starts = np.unique(rows, return_index=True)
        ends = np.append(starts[1:], len(rows))
        discount = 1.0 / np.log2(np.arange(2, k + 2))
        hits_total, m_total, ap_sum, ndcg_sum = 0.0, 0.0, 0.0, 0.0
        for b in range(0, len(users), batch):
            ids, _ = self.recommend(users[b:b + batch], k, True)
            for n, row in enumerate(ids):
                liked = set(cols[starts[b + n]:ends[b + n]].tolist())
                m = min(k, len(liked))
                hits, ap, dcg = 0, 0.0, 0.0
                for t, item in enumerate(row.tolist(), start=1):
                    if item >= 0 and item in liked:
                        hits += 1
                        ap += hits / t
                        dcg += discount[t - 1]
                hits_total += hits
                m_total += m
                ap_sum += ap / m
                ndcg_sum += dcg / discount[:m].sum()
        n_users = len(users)
        return dict(precision=float(hits_total / m_total) if m_total else 0.0, map=float(ap_sum / n_users) if n_users else 0.0,
                    ndcg=float(ndcg_sum / n_users) if n_users else 0.0, users=n_users)

    def _rank_of(self, users, items, filter_seen):
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int64).reshape(-1))
        items = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1))
        if len(users) != len(items):
            raise ValueError("rank_of needs as many users as items")
        ranks, candidates, in_seen = (np.empty(len(users), dtype=np.int64) for _ in range(3))
        _check(lib().hnh_ials_rank_of(self.h, users.ctypes.data, items.ctypes.data, len(users), int(bool(filter_seen)), ranks.ctypes.data,
                                      candidates.ctypes.data, in_seen.ctypes.data), "ials_rank_of")
        return ranks, candidates, in_seen

    def rank_of(self, users, items, filter_seen: bool = True):
        """The exact position of items[i] in users[i]'s full ordering of all N items by <a_u, b_j> (score descending, then item id
        ascending: recommend's order), for pairs in global coordinates, repeats allowed: (ranks int64 [n], candidates int64 [n]).
        ranks[i] counts the user's candidates other than items[i] that rank before it, 0-based: for an item the user has not seen it is
        the item's index in recommend(user, k = all, filter_seen).  candidates[i] is N, or with filter_seen (the items of the user's row
        of S are no candidates, the asked item always is) N - |seen_u \\ {items[i]}|: 0 <= ranks[i] < candidates[i].  Counted on the device
        from the scores' own bits: no score matrix is formed anywhere.  Collective: every rank passes the same pairs and gets the same
        arrays."""
        return self._rank_of(users, items, filter_seen)[:2]

    def rank_metrics(self, test_rows, test_cols, batch: int = 1024, filter_seen: bool = True) -> dict:
        """mpr, auc and mrr of held-out pairs in global coordinates (duplicates are dropped), the same on every rank, from rank_of's
        integers by host arithmetic; the users are ranked in batches of `batch`.  With L_u the held-out items of user u, h = |L_u|:
        mpr = the mean over the pairs of rank / (candidates - 1), 0 where candidates == 1: the expected percentile rank of Hu, Koren and
        Volinsky with r_ui = 1; 0 is best, 0.5 is random.
        auc = the mean over the users of 1 - (sum_t rank_t - h (h - 1) / 2) / (h neg), neg = N - |seen_u \\ L_u| - h the items that are
        neither seen nor held out (N - h without filter_seen): the share of (held-out, other) pairs that are ordered rightly.
        mrr = the mean over the users of 1 / (1 + min_t rank_t).
        A user with neg == 0 has nothing to be ranked against: it is left out of auc and mrr, and `users` counts the others; `pairs`
        counts every distinct pair.  The three sums are exactly rounded (math.fsum): they do not depend on `batch` or the pairs' order."""
        import math
        test_rows = np.asarray(test_rows, dtype=np.int64).reshape(-1)
        test_cols = np.asarray(test_cols, dtype=np.int64).reshape(-1)
        if len(test_rows) != len(test_cols) or batch < 1:
            raise ValueError("rank_metrics needs as many rows as columns and batch >= 1")
        pairs = np.unique(np.stack([test_rows, test_cols], axis=1), axis=0) if len(test_rows) else np.zeros((0, 2), np.int64)
        rows, cols = pairs[:, 0], pairs[:, 1]
        users, starts = np.unique(rows, return_index=True)
        ends = np.append(starts[1:], len(rows))
        pr, auc, rr = [], [], []
        for b in range(0, len(users), batch):
            lo, hi = int(starts[b]), int(ends[min(b + batch, len(users)) - 1])
            ranks, cand, in_seen = self._rank_of(rows[lo:hi], cols[lo:hi], filter_seen)
            pr += [r / (c - 1) if c > 1 else 0.0 for r, c in zip(ranks.tolist(), cand.tolist())]
            for u in range(b, min(b + batch, len(users))):
                s, e = int(starts[u]) - lo, int(ends[u]) - lo
                h = e - s
                neg = int(cand[s] - in_seen[s] + in_seen[s:e].sum()) - h
                if neg <= 0:
                    continue
                auc.append(1.0 - (int(ranks[s:e].sum()) - h * (h - 1) // 2) / (h * neg))
                rr.append(1.0 / (1 + int(ranks[s:e].min())))
        return dict(mpr=math.fsum(pr) / len(pr) if pr else 0.0, auc=math.fsum(auc) / len(auc) if auc else 0.0,
                    mrr=math.fsum(rr) / len(rr) if rr else 0.0, users=len(auc), pairs=len(pr))

    def free(self):
        if self.h:
            _check(lib().hnh_ials_destroy(self.h), "ials_destroy")
            self.h = None


class GAT:
    """GAT (gat.hpp): multi-head graph-attention forward pass on top of a DistributedSparse, and its backward pass (an addition)."""

    ATTENTION = {"none": 0, "softmax": 1}  # HNH_GAT_ATTENTION_NONE / _SOFTMAX

    BACKWARD = {"unfused": 0, "fused": 1}  # HNH_GAT_BACKWARD_UNFUSED / _FUSED

    SCORE = {"dot": 0, "additive": 1}  # HNH_GAT_SCORE_DOT / _ADDITIVE

    SCORE_V2 = {"gatv2": 2}  # HNH_GAT_SCORE_GATV2 (include/hnh_attn_v2.h); set_score accepts the union of the tables
    SCORE_QKV = {"transformer": 3}  # HNH_GAT_SCORE_TRANSFORMER (include/hnh_attn_qkv.h)
    EDGE_BIAS_ROW_MAX = 1e6  # edge_bias_from: the largest bias of a row of several edges lies within +-this (include/hnh_attn_edge.h, Magnitudes)

    ACTIVATION = {"relu": 0, "elu": 1, "identity": 2}  # HNH_GAT_ACT_RELU / _ELU / _IDENTITY

    RESIDUAL = {"none": 0, "identity": 1, "projection": 2}  # HNH_GAT_RESIDUAL_NONE / _IDENTITY / _PROJECTION

    NORM = {"none": 0, "layer": 1}  # HNH_GAT_NORM_NONE / _LAYER

    HEADS = {"mean": 0, "concat": 1}  # HNH_GAT_HEADS_MEAN / _CONCAT

    OPTIMIZER = {"adam": 0, "sgd": 1, "adamw": 2}  # HNH_GAT_OPTIMIZER_ADAM / _SGD / _ADAMW (the last: include/hnh_train_clip.h)

    LR_SCHEDULE = {"constant": 0, "linear": 1, "cosine": 2}  # HNH_GAT_LR_CONSTANT / _LINEAR / _COSINE

    def __init__(self, op: DistributedSparse, layers, leaky_relu_alpha: float = 0.2, attention: str = "none", backward: str = "unfused",
                 score: str = "dot", dropout=(0.0, 0.0), seed: int = 0, activation="relu", residual="none", bias=False, norm="none"):
        self.op, self.layers = op, [tuple(l) for l in layers]
        norms = [norm] * len(self.layers) if isinstance(norm, str) else list(norm)
        if len(norms) != len(self.layers):
            raise ValueError("norm is one name or one name per layer: %d layers, not %d names" % (len(self.layers), len(norms)))
        for n in norms:
            if n not in self.NORM:
                raise ValueError("norm must be one of %s, not %r" % (sorted(self.NORM), n))
        ress = [residual] * len(self.layers) if isinstance(residual, str) else list(residual)
        if len(ress) != len(self.layers):
            raise ValueError("residual is one name or one name per layer: %d layers, not %d names" % (len(self.layers), len(ress)))
        for r in ress:
            if r not in self.RESIDUAL:
                raise ValueError("residual must be one of %s, not %r" % (sorted(self.RESIDUAL), r))
        biases = [bool(bias)] * len(self.layers) if isinstance(bias, (bool, np.bool_)) else [bool(b) for b in bias]
        if len(biases) != len(self.layers):
            raise ValueError("bias is one flag or one flag per layer: %d layers, not %d flags" % (len(self.layers), len(biases)))
        acts = [activation] * len(self.layers) if isinstance(activation, str) else list(activation)
        if len(acts) != len(self.layers):
            raise ValueError("activation is one name or one name per layer: %d layers, not %d names" % (len(self.layers), len(acts)))
        for a in acts:
            if a not in self.ACTIVATION:
                raise ValueError("activation must be one of %s, not %r" % (sorted(self.ACTIVATION), a))
        spec = (C.c_int * (3 * len(layers)))(*[x for l in self.layers for x in l])
        self.h = _vp()
        _check(lib().hnh_gat_create(op.h, len(layers), spec, leaky_relu_alpha, C.byref(self.h)), "gat_create")
        if attention != "none":
            self.set_attention(attention)
        if backward != "unfused":
            self.set_backward(backward)
        if score != "dot":
            self.set_score(score)
        if tuple(dropout) != (0.0, 0.0) or seed != 0:
            self.set_dropout(dropout[0], dropout[1], seed)
        for i, a in enumerate(acts):
            if a != "relu":
                self.set_activation(i, a)
        try:
            for i, r in enumerate(ress):
                if r != "none":
                    self.set_residual(i, r)
            for i, b in enumerate(biases):
                if b:
                    self.set_bias(i, np.zeros(self.layers[i][1] * self.layers[i][2]))
            for i, n in enumerate(norms):
                if n != "none":
                    self.set_norm(i, n)
        except BaseException:
            self.free()
            raise

    def set_dropout(self, attention_p: float, feature_p: float, seed: int = 0):
        """Dropout rates in [0, 1) on the normalised attention coefficients (score "additive" only: not "dot", not "gatv2") and on every layer's input, with masks
        recomputed in every pass from Philox-4x32-10 keyed by (seed, layer, head, global row, global column)
        (include/hnh_attn_dropout.h): they do not depend on the rank count or the schedule's windows.  (0, 0), the default, runs the
        kernels without dropout at their widths.  Invalidates the stored forward pass; forwardPass raises HnhError where a rate is not
        supported."""
        for p in (attention_p, feature_p):
            if not (0.0 <= p < 1.0):
                raise ValueError("dropout rates must lie in [0, 1), not %r" % (p,))
        _check(lib().hnh_gat_set_dropout(self.h, float(attention_p), float(feature_p), int(seed) & 0xFFFFFFFFFFFFFFFF), "gat_set_dropout")

    def set_dropout_seed(self, seed: int):
        """New masks at the same rates (one call per training step).  Invalidates the stored forward pass."""
        _check(lib().hnh_gat_set_dropout_seed(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF), "gat_set_dropout_seed")

    def set_attention(self, mode: str):
        """"none" (the default: the LeakyReLU scores are the edge weights) or "softmax" (normalised over each row's neighbourhood;
        15d_fusion2 with c = 1 only, forwardPass raises HnhError elsewhere).  A change invalidates the stored forward pass."""
        if mode not in self.ATTENTION:
            raise ValueError("attention must be one of %s, not %r" % (sorted(self.ATTENTION), mode))
        _check(lib().hnh_gat_set_attention(self.h, self.ATTENTION[mode]), "gat_set_attention")

    def set_backward(self, mode: str):
        """"unfused" (the default: seven operator calls per head) or "fused" (two passes per head, include/hnh_attn_grad.h; 15d_fusion2
        with c = 1 and heads of at most 256 features only, backwardPass raises HnhError elsewhere).  Needs no new forward pass."""
        if mode not in self.BACKWARD:
            raise ValueError("backward must be one of %s, not %r" % (sorted(self.BACKWARD), mode))
        _check(lib().hnh_gat_set_backward(self.h, self.BACKWARD[mode]), "gat_set_backward")

    def set_score(self, mode: str):
        """"dot" (the default: e_ij = LeakyReLU(<A_i, A_j>)) or "additive" (e_ij = LeakyReLU(<A_i, a1> + <A_j, a2>) with the vectors of
        set_attention_vectors, include/hnh_attn_additive.h; attention "softmax" on 15d_fusion2 with c = 1 and heads of at most 256
        features only, forwardPass / backwardPass raise HnhError elsewhere), or "gatv2" (Brody, Alon and Yahav's dynamic attention,
        e_ij = sum_c a_c LeakyReLU(A_ic + A_jc) with ONE vector per head, the a1 of set_attention_vectors, include/hnh_attn_v2.h; supported
        where "additive" is, without attention dropout), or "transformer" (scaled dot-product attention with separate projections,
        s_ij = <Q_i, K_j> / sqrt(f) with Q = X W_q, K = X W_k and the aggregate over V = X W of set_weight, include/hnh_attn_qkv.h;
        set_query_weight / set_key_weight, zero until set, which is a stationary point: initialise them; supported where "gatv2" is).  With
        "additive", "gatv2" and "transformer" there is one backward implementation: set_backward is not consulted.  A change invalidates
        the stored forward pass."""
        table = dict(self.SCORE, **self.SCORE_V2, **self.SCORE_QKV)
        if mode not in table:
            raise ValueError("score must be one of %s, not %r" % (sorted(table), mode))
        _check(lib().hnh_gat_set_score(self.h, table[mode]), "gat_set_score")

    def set_activation(self, layer: int, mode: str):
        """"relu" (the default on every layer: out = max(o, 0)), "elu" (out = o for o > 0, expm1(o) otherwise) or "identity" (out = o) on the
        layer's output; the backward pass works from the stored output (include/hnh_grad.h, hnh_act_grad_cols_f64).  A non-ReLU layer needs
        attention "softmax" (score "dot" or "additive", any dropout rates) on 15d_fusion2 with c = 1: forwardPass / backwardPass /
        train_step / evaluate raise HnhError elsewhere, before anything is launched.  The published network is "elu" on the hidden layers
        and "identity" on the last with set_labels(heads="mean").  A change invalidates the stored forward pass."""
        if mode not in self.ACTIVATION:
            raise ValueError("activation must be one of %s, not %r" % (sorted(self.ACTIVATION), mode))
        if not (0 <= int(layer) < len(self.layers)):
            raise ValueError("layer %r out of range: %d layers" % (layer, len(self.layers)))
        _check(lib().hnh_gat_set_activation(self.h, int(layer), self.ACTIVATION[mode]), "gat_set_activation")

    # ---- bias and skip connections (include/hnh_gat_skip.h)
    def _layer(self, layer):
        if not (0 <= int(layer) < len(self.layers)):
            raise ValueError("layer %r out of range: %d layers" % (layer, len(self.layers)))
        return int(layer)

    def _width(self, layer):
        return self.layers[layer][1] * self.layers[layer][2]

    def set_residual(self, layer: int, mode: str):
        """The layer's skip connection, added before the activation: out = act(o + r + b) with r "none" (the default), "identity" (the layer
        input; needs input_features == heads * features_per_head) or "projection" (input @ W_res, W_res learned: set_residual_weight, zero
        until set).  Needs attention "softmax" (every score, both backward modes, any dropout the score allows, any activation) on
        15d_fusion2 with c = 1: forwardPass / backwardPass / train_step / evaluate raise HnhError elsewhere, before anything is launched.
        A change invalidates the stored forward pass."""
        if mode not in self.RESIDUAL:
            raise ValueError("residual must be one of %s, not %r" % (sorted(self.RESIDUAL), mode))
        _check(lib().hnh_gat_set_residual(self.h, self._layer(layer), self.RESIDUAL[mode]), "gat_set_residual")

    def set_residual_weight(self, layer: int, w: np.ndarray):
        """W_res of the layer: input_features x (heads * features_per_head), column block h belongs to head h.  Invalidates the stored
        forward pass like set_weight."""
        layer = self._layer(layer)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (self.layers[layer][0], self._width(layer)):
            raise ValueError("the residual weight of layer %d is %d x %d, not %r" % (layer, self.layers[layer][0], self._width(layer), w.shape))
        _check(lib().hnh_gat_set_residual_weight(self.h, layer, w.ctypes.data), "gat_set_residual_weight")

    def get_residual_weight(self, layer: int) -> np.ndarray:
        layer = self._layer(layer)
        out = np.empty((self.layers[layer][0], self._width(layer)))
        _check(lib().hnh_gat_get_residual_weight(self.h, layer, out.ctypes.data), "gat_get_residual_weight")
        return out

    def residual_weight_grad(self, layer: int) -> np.ndarray:
        """dL/dW_res of the layer after backwardPass with residual "projection", summed over every rank."""
        layer = self._layer(layer)
        out = np.empty((self.layers[layer][0], self._width(layer)))
        _check(lib().hnh_gat_get_residual_weight_grad(self.h, layer, out.ctypes.data), "gat_get_residual_weight_grad")
        return out

    def set_bias(self, layer: int, b):
        """The layer's learned bias (heads * features_per_head entries), added before the activation; None switches it off (the default).
        Supported where set_residual is.  Invalidates the stored forward pass."""
        layer = self._layer(layer)
        if b is None:
            _check(lib().hnh_gat_set_bias(self.h, layer, None), "gat_set_bias")
            return
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (self._width(layer),):
            raise ValueError("the bias of layer %d has %d entries, not shape %r" % (layer, self._width(layer), b.shape))
        _check(lib().hnh_gat_set_bias(self.h, layer, b.ctypes.data), "gat_set_bias")

    def get_bias(self, layer: int) -> np.ndarray:
        layer = self._layer(layer)
        out = np.empty(self._width(layer))
        _check(lib().hnh_gat_get_bias(self.h, layer, out.ctypes.data), "gat_get_bias")
        return out

    def bias_grad(self, layer: int) -> np.ndarray:
        """dL/db of the layer after backwardPass with a bias, summed over every rank."""
        layer = self._layer(layer)
        out = np.empty(self._width(layer))
        _check(lib().hnh_gat_get_bias_grad(self.h, layer, out.ctypes.data), "gat_get_bias_grad")
        return out

    # ---- layer normalisation (include/hnh_gat_norm.h)
    def set_norm(self, layer: int, mode: str, eps: float = 1e-5):
        """"none" (the default on every layer) or "layer": out = act(gamma * xh + beta) with xh = (z - mean(z)) / sqrt(var(z) + eps) over the
        WHOLE row z = o + r + b (all heads side by side; the biased variance), the post-norm block of the transformer and LayerNorm-then-
        activation of TransformerConv / UniMP.  gamma = 1 and beta = 0 until set_norm_weights; both are learned (norm_grad, optimizer_step,
        train_step) and never decayed.  A normalised layer keeps one more matrix of the layer output's size between the passes.  Needs
        attention "softmax" (every score, both backward modes, any dropout the score allows, bias and both residuals) on 15d_fusion2 with
        c = 1 and heads * features_per_head <= 4096: forwardPass / backwardPass / train_step / evaluate raise HnhError elsewhere, before
        anything is launched.  A change invalidates the stored forward pass."""
        if mode not in self.NORM:
            raise ValueError("norm must be one of %s, not %r" % (sorted(self.NORM), mode))
        eps = float(eps)
        if not (eps > 0.0 and np.isfinite(eps)):
            raise ValueError("the norm's eps must be positive and finite, not %r" % (eps,))
        _check(lib().hnh_gat_set_norm(self.h, self._layer(layer), self.NORM[mode], eps), "gat_set_norm")

    def _norm_pair(self, layer, gamma, beta, what):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        if gamma.shape != (self._width(layer),) or beta.shape != (self._width(layer),):
            raise ValueError("%s of layer %d have %d entries each, not shapes %r and %r" % (what, layer, self._width(layer), gamma.shape, beta.shape))
        return gamma, beta

    def set_norm_weights(self, layer: int, gamma, beta):
        """gamma and beta of the layer's norm (heads * features_per_head entries each).  Invalidates the stored forward pass like set_weight."""
        layer = self._layer(layer)
        gamma, beta = self._norm_pair(layer, gamma, beta, "gamma and beta")
        _check(lib().hnh_gat_set_norm_weights(self.h, layer, gamma.ctypes.data, beta.ctypes.data, gamma.size), "gat_set_norm_weights")

    def get_norm_weights(self, layer: int):
        """(gamma, beta) of the layer's norm as they stand: (ones, zeros) until set or trained."""
        layer = self._layer(layer)
        gamma, beta = np.empty(self._width(layer)), np.empty(self._width(layer))
        _check(lib().hnh_gat_get_norm_weights(self.h, layer, gamma.ctypes.data, beta.ctypes.data, gamma.size), "gat_get_norm_weights")
        return gamma, beta

    def norm_grad(self, layer: int):
        """(dL/dgamma, dL/dbeta) of the layer after backwardPass with the layer normalised, summed over every rank."""
        layer = self._layer(layer)
        dgamma, dbeta = np.empty(self._width(layer)), np.empty(self._width(layer))
        _check(lib().hnh_gat_get_norm_grad(self.h, layer, dgamma.ctypes.data, dbeta.ctypes.data, dgamma.size), "gat_get_norm_grad")
        return dgamma, dbeta

    def set_attention_vectors(self, layer: int, head: int, a1: np.ndarray, a2: np.ndarray):
        """The additive score's vectors of (layer, head): features_per_head entries each, zero until set.  Score "gatv2" uses a1 as the
        head's one vector and keeps a2 without reading it.  Invalidates the stored forward pass like set_weight."""
        f = self.layers[layer][1]
        a1 = np.ascontiguousarray(a1, dtype=np.float64)
        a2 = np.ascontiguousarray(a2, dtype=np.float64)
        assert a1.shape == (f,) and a2.shape == (f,)
        _check(lib().hnh_gat_set_attn_vectors(self.h, layer, head, a1.ctypes.data, a2.ctypes.data), "gat_set_attn_vectors")

    def attention_grad(self, layer: int, head: int):
        """(dL/da1, dL/da2) of (layer, head) after backwardPass with score "additive", summed over every rank; with score "gatv2"
        (dL/da, zeros)."""
        f = self.layers[layer][1]
        da1, da2 = np.empty(f), np.empty(f)
        _check(lib().hnh_gat_get_attn_grads(self.h, layer, head, da1.ctypes.data, da2.ctypes.data), "gat_get_attn_grads")
        return da1, da2

    def weight_shape(self, layer: int, head: int):
        o = (C.c_int64 * 2)()
        _check(lib().hnh_gat_weight_shape(self.h, layer, head, o), "gat_weight_shape")
        return int(o[0]), int(o[1])

    def set_weight(self, layer: int, head: int, w: np.ndarray):
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == self.weight_shape(layer, head)
        _check(lib().hnh_gat_set_weight(self.h, layer, head, w.ctypes.data), "gat_set_weight")

    # ---- the transformer score's query and key weights (include/hnh_attn_qkv.h): which = 0 is W_q, 1 is W_k
    def _set_qk(self, layer, head, which, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != self.weight_shape(layer, head):
            raise ValueError("the weight of layer %d, head %d is %r, not %r" % (layer, head, self.weight_shape(layer, head), w.shape))
        _check(lib().hnh_gat_set_qk_weight(self.h, int(layer), int(head), which, w.ctypes.data), "gat_set_qk_weight")

    def _get_qk(self, fn, name, layer, head, which):
        out = np.empty(self.weight_shape(layer, head))
        _check(fn(self.h, int(layer), int(head), which, out.ctypes.data), name)
        return out

    def set_query_weight(self, layer: int, head: int, w: np.ndarray):
        """W_q of (layer, head) for score "transformer": the shape of set_weight's, zero until set.  Invalidates the stored forward pass."""
        self._set_qk(layer, head, 0, w)

    def set_key_weight(self, layer: int, head: int, w: np.ndarray):
        """W_k of (layer, head) for score "transformer": the shape of set_weight's, zero until set.  Invalidates the stored forward pass."""
        self._set_qk(layer, head, 1, w)

    def get_query_weight(self, layer: int, head: int) -> np.ndarray:
        return self._get_qk(lib().hnh_gat_get_qk_weight, "gat_get_qk_weight", layer, head, 0)

    def get_key_weight(self, layer: int, head: int) -> np.ndarray:
        return self._get_qk(lib().hnh_gat_get_qk_weight, "gat_get_qk_weight", layer, head, 1)

    def query_weight_grad(self, layer: int, head: int) -> np.ndarray:
        """dL/dW_q of (layer, head) after backwardPass with score "transformer", summed over every rank."""
        return self._get_qk(lib().hnh_gat_get_qk_weight_grad, "gat_get_qk_weight_grad", layer, head, 0)

    def key_weight_grad(self, layer: int, head: int) -> np.ndarray:
        """dL/dW_k of (layer, head) after backwardPass with score "transformer", summed over every rank."""
        return self._get_qk(lib().hnh_gat_get_qk_weight_grad, "gat_get_qk_weight_grad", layer, head, 1)

    # ---- the per-edge bias of the transformer score's logits (include/hnh_attn_edge.h)
    def set_edge_bias(self, layer: int, bias_s: Vec | None, bias_st: Vec | None):
        """A per-edge bias on layer `layer`'s logits with score "transformer": s_ij = <Q_i, K_j> / sqrt(f) + b_ij, one finite value per nonzero
        of S on this rank, shared by the layer's heads and not learned (b = log w: the weighted neighbourhood softmax; a distance or relation
        bias; -1e300 removes an edge from every row that keeps one of moderate bias; -inf is not supported; a row's largest bias should stay
        within +-EDGE_BIAS_ROW_MAX, and a row of several edges that are all switched off is not supported: include/hnh_attn_edge.h, which
        this call does not check and edge_bias_from does).  bias_s is in the like_S_values layout and
        bias_st holds the same values in the like_ST_values layout (edge_bias_from builds both from one function); both are copied.  Both
        None clears the bias: the layer launches what it launched before.  HnhError for one None, a wrong length or a layer out of range,
        which leave the object as it was.  Invalidates the stored forward pass; any other score refuses a layer with an edge bias when a pass
        is asked for."""
        _check(lib().hnh_gat_set_edge_bias(self.h, int(layer), bias_s.h if bias_s is not None else None, bias_st.h if bias_st is not None else None),
               "gat_set_edge_bias")

    def edge_bias_from(self, fn, layer: int | None = None):
        """set_edge_bias from one function: fn(rows, cols) -> float64 array gives the bias of the nonzeros at the global coordinates (rows, cols)
        of S; it is evaluated on op.S_coordinates() and on op.ST_coordinates() (swapped back to the coordinates of S), uploaded in both layouts and
        set on `layer`, or on every layer when None.  A function of the coordinates alone gives the two layouts the same values, which is what
        the backward pass needs.  ValueError for a value that is not finite, and for a row of two or more entries whose largest bias lies
        beyond +-EDGE_BIAS_ROW_MAX (such as a row whose every edge is switched off with -1e300): the backward pass recomputes the
        coefficients from the row's lse, which is as large as that bias, and would lose them (include/hnh_attn_edge.h); a single edge may
        carry any finite value.  Collective, like S_coordinates."""
        made = []
        try:
            for transposed, like in ((False, self.op.like_S_values), (True, self.op.like_ST_values)):
                if transposed:  # (an entry (j, i) of S^T is the nonzero (i, j) of S)
                    cols, rows = self.op.ST_coordinates()
                else:
                    rows, cols = self.op.S_coordinates()
                vals = np.ascontiguousarray(np.broadcast_to(np.asarray(fn(rows, cols), dtype=np.float64), rows.shape))
                if not np.all(np.isfinite(vals)):
                    raise ValueError("an edge bias must be finite (use a very negative value such as -1e300 to switch an edge off)")
                if not transposed and len(rows):  # (15d_fusion2 with c = 1, the only schedule that runs a bias, keeps whole rows of S on a rank)
                    ids, inv, deg = np.unique(rows, return_inverse=True, return_counts=True)
                    top = np.full(len(ids), -np.inf)
                    np.maximum.at(top, inv, vals)
                    bad = np.flatnonzero((deg >= 2) & (np.abs(top) > self.EDGE_BIAS_ROW_MAX))
                    if len(bad):
                        raise ValueError("the largest edge bias of row %d is %g: a row of several edges needs one within +-%g (a row whose every "
                                         "edge is switched off is not supported)" % (ids[bad[0]], top[bad[0]], self.EDGE_BIAS_ROW_MAX))
                v = like(0.0)
                made.append(v)
                v.upload(vals)
            for i in (range(len(self.layers)) if layer is None else [int(layer)]):
                self.set_edge_bias(i, made[0], made[1])
        finally:
            for v in made:
                v.free()

    # ---- a learned edge bias (include/hnh_attn_edge_grad.h)
    def set_edge_bias_learned(self, layer: int, on: bool = True):
        """Makes layer `layer`'s edge bias a parameter (or, with on=False, a constant again): backwardPass then also computes
        dL/db_e = sum_h p_e (<dZ_i, V_j> - delta_i) per nonzero, and optimizer_step / train_step update the bias from it with the other
        parameters' hyper-parameters but never with weight decay, so an entry at -1e300 keeps gradient 0 and stays -1e300 to the bit.  Both
        copies of the bias (like_S_values and like_ST_values order) are parameters, each updated from its own pass's gradient; every rank
        holds its own nonzeros' bias and nothing is all-reduced.  HnhError unless the layer has an edge bias; clearing the bias clears the
        switch."""
        _check(lib().hnh_gat_set_edge_bias_learned(self.h, int(layer), 1 if on else 0), "gat_set_edge_bias_learned")

    def _edge_vectors(self, fn, name, layer):
        out = []
        for which, like in ((0, self.op.like_S_values), (1, self.op.like_ST_values)):
            v = like(0.0)
            try:
                _check(fn(self.h, int(layer), which, v.h), name)
                out.append(v.download())
            finally:
                v.free()
        return tuple(out)

    def get_edge_bias(self, layer: int):
        """(bias_s, bias_st): layer `layer`'s edge bias as it stands on this rank, in the like_S_values and the like_ST_values layout."""
        return self._edge_vectors(lib().hnh_gat_get_edge_bias, "gat_get_edge_bias", layer)

    def edge_bias_grad(self, layer: int):
        """(dbias_s, dbias_st): dL/db of layer `layer`'s learned edge bias after backwardPass, per nonzero of S on this rank in the
        like_S_values layout (from the backward row pass) and in the like_ST_values layout (from the column pass); not summed over ranks,
        which hold different nonzeros.  HnhError before a backward pass with the bias learned."""
        return self._edge_vectors(lib().hnh_gat_get_edge_bias_grad, "gat_get_edge_bias_grad", layer)

    def buffer_shape(self, index: int):
        o = (C.c_int64 * 2)()
        _check(lib().hnh_gat_buffer_shape(self.h, index, o), "gat_buffer_shape")
        return int(o[0]), int(o[1])

    def set_input(self, x: Dense):
        _check(lib().hnh_gat_set_input(self.h, x.h), "gat_set_input")

    def get_output(self, out: Dense):
        _check(lib().hnh_gat_get_output(self.h, out.h), "gat_get_output")

    def forwardPass(self):
        _check(lib().hnh_gat_forward(self.h), "forwardPass")

    def backwardPass(self, grad_out: Dense):
        """Gradients of L from grad_out = dL/d(output) (the layout of get_output): needs a forwardPass since the last set_weight /
        set_input; 15d_fusion1 and 15d_fusion2 with c = 1 only (HnhError otherwise)."""
        _check(lib().hnh_gat_backward(self.h, grad_out.h), "backwardPass")

    def attention_coefficients(self, layer: int, head: int, out: Vec | None = None, dropped: bool = False) -> Vec:
        """The attention coefficients a_ij = exp(z_ij - lse_i) of (layer, head) of the stored forward pass, one per nonzero of S on this
        rank, in the like_S_values layout (op.S_coordinates() gives every entry's global row and column); every score mode
        (include/hnh_attn_coef.h).  dropped=True under a nonzero attention dropout rate: c m_ij a_ij, the weights the aggregate used;
        dropped=False always gives the normalised a_ij over all edges.  `out` is allocated with op.like_S_values when None.  Needs a
        forwardPass since the last set_weight / set_input / optimizer_step and attention "softmax" (15d_fusion2 with c = 1, heads of at
        most 256 features): HnhError elsewhere, before anything is launched.  Leaves the stored pass, the gradients, the seed and the
        optimizer state as they are."""
        made = out is None
        if made:
            out = self.op.like_S_values(0.0)
        try:
            _check(lib().hnh_gat_attention_coefficients(self.h, int(layer), int(head), int(bool(dropped)), out.h), "gat_attention_coefficients")
        except BaseException:
            if made:
                out.free()
            raise
        return out

    def weight_grad(self, layer: int, head: int) -> np.ndarray:
        """dL/dW of (layer, head) after backwardPass, summed over every rank (the same on all of them)."""
        out = np.empty(self.weight_shape(layer, head))
        _check(lib().hnh_gat_get_weight_grad(self.h, layer, head, out.ctypes.data), "gat_get_weight_grad")
        return out

    def get_input_grad(self, dx: Dense):
        """dL/d(input) after backwardPass, in the layout of buffer 0 (set_input's)."""
        _check(lib().hnh_gat_get_input_grad(self.h, dx.h), "gat_get_input_grad")

    # ---- training (include/hnh_train.h)
    def get_weight(self, layer: int, head: int) -> np.ndarray:
        out = np.empty(self.weight_shape(layer, head))
        _check(lib().hnh_gat_get_weight(self.h, layer, head, out.ctypes.data), "gat_get_weight")
        return out

    def get_attention_vectors(self, layer: int, head: int):
        """(a1, a2) of (layer, head): zero until set or trained."""
        f = self.layers[layer][1]
        a1, a2 = np.empty(f), np.empty(f)
        _check(lib().hnh_gat_get_attn_vectors(self.h, layer, head, a1.ctypes.data, a2.ctypes.data), "gat_get_attn_vectors")
        return a1, a2

    def _mask(self, mask):
        if mask is None:
            return None, 0
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.ndim != 1:
            raise ValueError("a mask is a one-dimensional array with one entry per global row")
        return m, len(m)

    def set_labels(self, labels, train_mask=None, heads: str = "mean"):
        """Class labels and the training mask: host arrays with one entry per global row of the operator (the numbering of get_output's
        rows); a negative label or a row outside the mask is not in the loss.  heads "mean": the logits are the mean over the last
        layer's heads (features_per_head classes); "concat": the row as it is (num_heads * features_per_head classes).  Each rank keeps
        its slice on the device; collective.  A label out of range, a mask without a labelled row or a wrong length raises."""
        if heads not in self.HEADS:
            raise ValueError("heads must be one of %s, not %r" % (sorted(self.HEADS), heads))
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 1:
            raise ValueError("labels is a one-dimensional array with one entry per global row")
        m, n = self._mask(train_mask)
        if m is not None and n != len(lab):
            raise ValueError("labels and train_mask differ in length: %d and %d" % (len(lab), n))
        _check(lib().hnh_gat_set_labels(self.h, lab.ctypes.data, None if m is None else m.ctypes.data, len(lab), self.HEADS[heads]), "gat_set_labels")

    def set_multilabel_targets(self, targets, train_mask=None, heads: str = "mean", pos_weight=None):
        """Multi-label targets: a bool or 0/1 host array of shape (M, classes) in the operator's global row numbering, where classes is
        what `heads` gives ("mean": the last layer's features_per_head; "concat": num_heads * features_per_head); train_mask selects the
        rows of the loss (None: every row); pos_weight holds one weight >= 0 per class for its positive term (None: 1), as in
        BCEWithLogitsLoss(pos_weight=...).  Afterwards loss / train_step / evaluate use the sigmoid head (include/hnh_train_multilabel.h)
        until the next set_labels: the most recent of the two calls decides.  Each rank keeps its rows' bits on the device; collective.
        Any other target value, a class count that does not match, a mask that selects no row or a bad weight raises and leaves the
        object as it was."""
        if heads not in self.HEADS:
            raise ValueError("heads must be one of %s, not %r" % (sorted(self.HEADS), heads))
        t = np.asarray(targets)
        if t.ndim != 2:
            raise ValueError("targets is a two-dimensional array of shape (global rows, classes)")
        bad = np.argwhere(~((t == 0) | (t == 1)))  # (before the cast to bytes, which would fold 256 onto 0; the host layer checks the bytes again)
        if len(bad):
            raise ValueError("target %r of row %d, class %d is neither 0 nor 1" % (t[tuple(bad[0])].item(), bad[0][0], bad[0][1]))
        t = np.ascontiguousarray(t, dtype=np.uint8)
        m, n = self._mask(train_mask)
        if m is not None and n != t.shape[0]:
            raise ValueError("targets and train_mask differ in length: %d and %d" % (t.shape[0], n))
        pw = None
        if pos_weight is not None:
            pw = np.ascontiguousarray(pos_weight, dtype=np.float64)
            if pw.shape != (t.shape[1],):
                raise ValueError("pos_weight needs one entry per class: shape (%d,), not %r" % (t.shape[1], pw.shape))
        _check(lib().hnh_gat_set_multilabel_targets(self.h, t.ctypes.data, t.size, t.shape[1], None if m is None else m.ctypes.data, n, self.HEADS[heads],
                                                    None if pw is None else pw.ctypes.data), "gat_set_multilabel_targets")

    def multilabel_counts(self):
        """(tp, fp, fn) of the last loss / evaluate / train_step under the sigmoid head: exact counts of (row, class) pairs over the whole
        world, the prediction being logit > 0."""
        tp, fp, fn = C.c_double(), C.c_double(), C.c_double()
        _check(lib().hnh_gat_multilabel_counts(self.h, C.byref(tp), C.byref(fp), C.byref(fn)), "gat_multilabel_counts")
        return int(tp.value), int(fp.value), int(fn.value)

    def loss(self, mask=None, grad_out: Dense | None = None):
        """The pair of the stored forward pass over the rows of `mask` (None: the training rows), over the whole world.  After set_labels:
        (loss, accuracy), the mean softmax cross-entropy over the labelled rows and the share of them whose argmax is the label.  After
        set_multilabel_targets: (loss, micro-F1), the mean weighted sigmoid cross-entropy over selected rows x classes and 2 tp / (2 tp +
        fp + fn) of the prediction logit > 0 (0.0 when the denominator is 0; multilabel_counts() has the counts).  grad_out receives
        dL/d(output), which backwardPass takes."""
        m, n = self._mask(mask)
        lo, acc = C.c_double(), C.c_double()
        _check(lib().hnh_gat_loss(self.h, None if m is None else m.ctypes.data, n, grad_out.h if grad_out is not None else None, C.byref(lo), C.byref(acc)),
               "gat_loss")
        return lo.value, acc.value

    def set_optimizer(self, kind: str, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, momentum: float = 0.0,
                      weight_decay: float = 0.0):
        """"adam", "sgd" (with momentum) or "adamw" over every W, a1, a2 with score "additive", and every enabled bias and residual weight;
        with "adam" and "sgd" weight decay is added to the gradient of each of them, with "adamw" it shrinks the parameter itself by
        lr * weight_decay before Adam's update (torch.optim.AdamW; include/hnh_train_clip.h).  A learned edge bias
        (set_edge_bias_learned) is updated too, but never decayed.  (Re)allocates zeroed moments and resets the step count; the clip
        setting (set_grad_clip) and the schedule (set_lr_schedule) stay in place."""
        if kind not in self.OPTIMIZER:
            raise ValueError("optimizer must be one of %s, not %r" % (sorted(self.OPTIMIZER), kind))
        _check(lib().hnh_gat_set_optimizer(self.h, self.OPTIMIZER[kind], float(lr), float(beta1), float(beta2), float(eps), float(momentum),
                                           float(weight_decay)), "gat_set_optimizer")

    def set_grad_clip(self, max_norm: float | None):
        """Gradient clipping by global norm, on the device (include/hnh_train_clip.h): every later optimizer_step / train_step scales all
        gradients by min(1, max_norm / (norm + 1e-6)), norm being the 2-norm over every learned tensor of the whole world, as
        torch.nn.utils.clip_grad_norm_ does.  train_step keeps its single host synchronisation.  None or 0 switches clipping off (the
        default); a value that is negative, NaN or infinite raises and leaves the object as it was."""
        _check(lib().hnh_gat_set_grad_clip(self.h, 0.0 if max_norm is None else float(max_norm)), "gat_set_grad_clip")

    def grad_norm(self) -> float:
        """The global gradient norm, before clipping, of the most recent optimizer_step / train_step taken with clipping on (a copy
        and a host synchronisation of its own).  Raises before the first such step."""
        out = C.c_double()
        _check(lib().hnh_gat_grad_norm(self.h, C.byref(out)), "gat_grad_norm")
        return out.value

    def set_learning_rate(self, lr: float):
        """A new base learning rate; unlike set_optimizer it keeps the moments and the step count."""
        _check(lib().hnh_gat_set_learning_rate(self.h, float(lr)), "gat_set_learning_rate")

    def learning_rate(self) -> float:
        """The rate the next optimizer_step / train_step will use: the base rate times the schedule's factor."""
        out = C.c_double()
        _check(lib().hnh_gat_learning_rate(self.h, C.byref(out)), "gat_learning_rate")
        return out.value

    def set_lr_schedule(self, kind: str = "constant", warmup_steps: int = 0, total_steps: int = 0, min_factor: float = 0.0):
        """lr_t = lr * factor(t) for the 1-based step t: t / warmup_steps during the warm-up; afterwards "constant" gives 1 (total_steps
        and min_factor are not used), "linear" 1 - (1 - min_factor) (t - W) / (T - W) and "cosine" min_factor + (1 - min_factor)
        (1 + cos(pi (t - W) / (T - W))) / 2, and min_factor beyond total_steps.  "linear" and "cosine" need total_steps > warmup_steps
        >= 0 and min_factor in [0, 1]; anything else raises.  set_optimizer restarts t and keeps the schedule."""
        if kind not in self.LR_SCHEDULE:
            raise ValueError("schedule must be one of %s, not %r" % (sorted(self.LR_SCHEDULE), kind))
        _check(lib().hnh_gat_set_lr_schedule(self.h, self.LR_SCHEDULE[kind], int(warmup_steps), int(total_steps), float(min_factor)), "gat_set_lr_schedule")

    def optimizer_step(self):
        """One optimizer step from the gradients of the last backwardPass, on the device.  Invalidates the stored forward pass."""
        _check(lib().hnh_gat_optimizer_step(self.h), "gat_optimizer_step")

    def train_step(self):
        """Forward pass, loss over the training rows, backward pass and optimizer step on the device; returns the pair of the parameters
        before the update, the call's only host synchronisation: (loss, accuracy) after set_labels, (loss, micro-F1) after
        set_multilabel_targets, as loss() defines them.  With a nonzero dropout rate the seed advances by one first: step t of a run
        uses the masks of seed + t."""
        lo, acc = C.c_double(), C.c_double()
        _check(lib().hnh_gat_train_step(self.h, C.byref(lo), C.byref(acc)), "gat_train_step")
        return lo.value, acc.value

    def evaluate(self, mask=None):
        """The pair over the rows of `mask` (None: the training rows) from a forward pass without dropout and without a gradient:
        (loss, accuracy) over the labelled rows after set_labels, (loss, micro-F1) over the selected rows x classes after
        set_multilabel_targets, as loss() defines them; rates and seed are as before afterwards."""
        m, n = self._mask(mask)
        lo, acc = C.c_double(), C.c_double()
        _check(lib().hnh_gat_evaluate(self.h, None if m is None else m.ctypes.data, n, C.byref(lo), C.byref(acc)), "gat_evaluate")
        return lo.value, acc.value

    def free(self):
        if self.h:
            _check(lib().hnh_gat_destroy(self.h), "gat_destroy")
            self.h = None
